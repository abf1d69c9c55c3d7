"""Operands, references and gates for fplll_amd/csrc/ftx.h (double-double DD, quad-double QD), shared by the host
check (tests/test_ftx_cpu.py: the header compiled by g++) and the device check (tests/test_ftx_gpu.py: the same
header inside libfplll_hip.so), so that both see the SAME operands and the device result can also be compared bit for
bit with the host's.  Deterministic from a seed.  Every reference is multiprecision (mpmath) or exact (integers).

An operand is a row of four doubles x[0..4) whose exact sum is the value (x[2], x[3] are zero for DD).  Operands are
normalised — x[k+1] is what rounding the remainder to nearest leaves, |x[k+1]| <= ulp(x[k]) / 2 — except the class
"gap", which is a valid non-overlapping expansion with a zero in the middle, as a caller could hand one in.

Classes of (a, b) pairs, cycling over the index:
  random   four (two) non-zero components, magnitudes 2^-30 .. 2^30
  int62    62-bit integers: the value ends inside x[1], everything below is exactly zero
  cancel   b = -a (1 + 2^-k), k in 20 .. 190: a + b cancels k bits
  equal    b = a
  plain    plain doubles, x[1..] = 0
  far      magnitudes 2^60 .. 2^260 apart
  gap      x[1] = 0 and x[2] != 0 (QD; for DD this is "plain")
  pow2     a power of two against 2^k - 2^-150 (the binade boundary: ulp changes between a and b)
  scaled   "random" with the exponents moved by 2^+-(200 .. 400) — the same way for both operands, in opposite
           directions for the products (variant "mul"): below 2^-1022 the error term of a product is not
           representable, in libqd as here, and that is not what is being checked
"""
import functools
import os
import subprocess

import numpy as np

try:
    import mpmath as mp
except ImportError:  # the tests importorskip mpmath before they call anything here
    mp = None

PREC = 900
CLASSES = ("random", "int62", "cancel", "equal", "plain", "far", "gap", "pow2", "scaled")
EPS_BITS = {2: 104, 4: 205}   # the unit of the gates: 2^-104 for DD, 2^-205 for QD
# op -> (name, tolerance in units); the tolerances tests/test_ftx_cpu.py has always used.  add / sub ("sloppy"
# addition): relative to the larger operand; the others: relative to the result.
ARITH = {0: ("add", 1), 1: ("sub", 1), 2: ("mul", 4), 3: ("div", 8), 4: ("sqrt", 4), 6: ("mul by a double", 4)}


def split(v, comps):
    """the normalised expansion of the mpf v: round to nearest, subtract, repeat"""
    x = [0.0] * 4
    for k in range(comps):
        x[k] = float(v)
        v = v - mp.mpf(x[k])
    return x


def val(x):
    return mp.fsum(mp.mpf(float(t)) for t in x)


def _rand_val(rng, comps, lo=-30, hi=30):
    v = mp.mpf(float(rng.standard_normal())) * mp.mpf(2) ** int(rng.integers(lo, hi))
    for k in range(1, comps):
        v = v * (1 + mp.mpf(float(rng.uniform(-1, 1))) * mp.mpf(2) ** (-55 * k))
    return v


def _sign(rng):
    return 1 if rng.integers(2) else -1


@functools.lru_cache(maxsize=None)
def _arith(seed, comps, n):
    mp.mp.prec = PREC
    rng = np.random.default_rng(seed)
    a, b = np.zeros((n, 4)), np.zeros((n, 4))
    cls, shift = [], np.zeros(n, dtype=np.int64)
    for i in range(n):
        c = CLASSES[i % len(CLASSES)]
        cls.append(c)
        if c in ("random", "scaled"):
            a[i], b[i] = split(_rand_val(rng, comps), comps), split(_rand_val(rng, comps), comps)
            if c == "scaled":
                shift[i] = _sign(rng) * int(rng.integers(200, 401))
        elif c == "int62":
            a[i] = split(mp.mpf(_sign(rng) * int(rng.integers(1 << 61, 1 << 62))), comps)
            b[i] = split(mp.mpf(_sign(rng) * int(rng.integers(1 << 61, 1 << 62))), comps)
        elif c == "cancel":
            va = val(split(_rand_val(rng, comps), comps))
            a[i], b[i] = split(va, comps), split(-va * (1 + mp.mpf(2) ** -int(rng.integers(20, 191))), comps)
        elif c == "equal":
            a[i] = split(_rand_val(rng, comps), comps)
            b[i] = a[i]
        elif c == "plain" or (c == "gap" and comps == 2):
            a[i, 0], b[i, 0] = float(_rand_val(rng, 1)), float(_rand_val(rng, 1))
        elif c == "far":
            va = _rand_val(rng, comps)
            vb = _rand_val(rng, comps, 0, 1) * mp.mpf(2) ** (int(mp.floor(mp.log(abs(va), 2))) +
                                                              _sign(rng) * int(rng.integers(60, 261)))
            a[i], b[i] = split(va, comps), split(vb, comps)
        elif c == "gap":
            for x in (a, b):
                x0 = float(_rand_val(rng, 1))
                low = split(_rand_val(rng, 2, 0, 1) * mp.mpf(2) ** (int(np.frexp(x0)[1]) - int(rng.integers(110, 150))), 2)
                x[i] = [x0, 0.0, low[0], low[1]]
        elif c == "pow2":
            j, k = int(rng.integers(-30, 31)), int(rng.integers(-30, 31))
            if rng.integers(2):
                k = j                                  # half of them meet at the same binade boundary
            sa, sb = _sign(rng), _sign(rng)
            a[i], b[i] = split(sa * mp.mpf(2) ** j, comps), split(sb * (mp.mpf(2) ** k - mp.mpf(2) ** -150), comps)
            if rng.integers(2):
                a[i], b[i] = b[i].copy(), a[i].copy()
    for x in (a, b):
        x.setflags(write=False)
    shift.setflags(write=False)
    return a, b, tuple(cls), shift


def arith_cases(seed, comps, n, variant="add"):
    """(a, b, cls): [n][4] operand planes of the classes above and the class name of every pair.  variant "mul": the
    class "scaled" moves b's exponent the other way (see the module docstring)."""
    a0, b0, cls, shift = _arith(seed, comps, n)
    a, b = np.ldexp(a0, shift[:, None]), np.ldexp(b0, (-shift if variant == "mul" else shift)[:, None])
    return a, b, cls


def nint_cases(seed, comps, n):
    """operands for nint: general ones up to 2^140; integral leading components (the next one decides, and the one
    after it when that is integral too); exact .5 ties of a component that a later component breaks either way, or
    nothing breaks (then the tie goes up, like libqd's nint); |x| >= 2^52, where every leading component is integral."""
    mp.mp.prec = PREC
    rng = np.random.default_rng(seed)
    q = np.zeros((n, 4))
    for i in range(n):
        k = i % 6
        if k == 0:
            v = _rand_val(rng, comps, 0, 140)
        elif k == 1:    # integral leading component, the rest small
            v = mp.mpf(int(rng.integers(-(1 << 40), 1 << 40))) + _rand_val(rng, comps, -60, 0)
        elif k == 2:    # tie of the leading component, broken up or down by something far below — or by nothing
            v = mp.mpf(int(rng.integers(-(1 << 30), 1 << 30))) + mp.mpf(1) / 2
            v += [0, 1, -1][int(rng.integers(3))] * abs(_rand_val(rng, comps - 1, -90, -60))
        elif k == 3:    # |x| >= 2^52: the fraction lives in x[1] (and x[2])
            v = mp.mpf(_sign(rng) * int(rng.integers(1 << 52, 1 << 62))) + _rand_val(rng, comps - 1, -40, 2)
        elif k == 4:    # leading component integral, the SECOND one a tie, broken (QD) or not
            v = mp.mpf(_sign(rng) * int(rng.integers(1 << 53, 1 << 60))) * 1024 + \
                mp.mpf(int(rng.integers(-500, 500))) + mp.mpf(1) / 2
            if comps == 4:
                v += [0, 1, -1][int(rng.integers(3))] * abs(_rand_val(rng, 2, -80, -60))
        else:           # an integer already
            v = mp.mpf(_sign(rng) * int(rng.integers(1, 1 << 62))) * 2 ** int(rng.integers(0, 60))
        q[i] = split(v, comps)
    return q


def cmp_cases(seed, comps, n):
    """pairs for f_le / f_gt: the arithmetic classes, pairs equal in every component, and pairs that differ in the
    last component only (by one ulp of it)"""
    a, b, cls = arith_cases(seed, comps, n)
    a, b, cls = a.copy(), b.copy(), list(cls)
    rng = np.random.default_rng(seed + 1)
    for i in range(0, n, 4):
        mp.mp.prec = PREC
        a[i] = split(_rand_val(rng, comps), comps)
        b[i] = a[i]
        cls[i] = "equal"
        if i % 8 == 0:
            b[i, comps - 1] = np.nextafter(a[i, comps - 1], [np.inf, -np.inf][(i // 8) % 2])
            cls[i] = "last"
    return a, b, tuple(cls)


def rnd_we_cases(seed, comps, n):
    """(a, e): the arithmetic operands with shifts e in -40 .. 70, so that both branches of rnd_we are taken"""
    a, _, cls = arith_cases(seed, comps, n)
    rng = np.random.default_rng(seed + 2)
    e = np.zeros((n, 4))
    e[:, 0] = rng.integers(-40, 71, n)
    return a, e, cls


def wave_cases(seed, comps, n_waves):
    """[64 * n_waves][4] operands for f_wave_sum: waves of mixed signs and magnitudes; wave 1: 63 zeros and one value;
    wave 2: exact cancellation (every odd lane is minus its even neighbour: the two halves of the last butterfly
    level are mirror images)."""
    mp.mp.prec = PREC
    rng = np.random.default_rng(seed)
    a = np.zeros((64 * n_waves, 4))
    for i in range(64 * n_waves):
        a[i] = split(_rand_val(rng, comps, -30 if (i // 64) % 2 else -3, 30 if (i // 64) % 2 else 3), comps)
    a[64:128] = 0.0
    a[64 + 37] = split(_rand_val(rng, comps), comps)
    a[129:192:2] = -a[128:192:2]
    return a


# ---- the host build of the header ---------------------------------------------------------------------------------
def host_harness(tmpdir):
    """tests/native/ftx_host.cpp compiled with the library's floating-point flags (no contraction, no fast-math);
    returns run(comps, op, a, b) -> [n][4] result planes"""
    exe = os.path.join(str(tmpdir), "ftx_host")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "ftx_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src])

    def run(comps, op, a, b):
        code = op + (10 if comps == 2 else 0)
        inp = "\n".join("%d %s %s" % (code, " ".join(float(t).hex() for t in a[i]), " ".join(float(t).hex() for t in b[i]))
                        for i in range(len(a)))
        res = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.strip().split("\n")
        assert len(res) == len(a)
        out = np.zeros((len(a), 4))
        for i, l in enumerate(res):
            t = [float.fromhex(w) for w in l.split()]
            out[i, :len(t)] = t
        return out
    return run


# ---- references and gates -------------------------------------------------------------------------------------
def reference(op, x, y):
    return {0: lambda: x + y, 1: lambda: x - y, 2: lambda: x * y, 3: lambda: x / y, 4: lambda: mp.sqrt(x),
            6: lambda: x * y}[op]()


def arith_error(comps, op, a, b, out):
    """worst error of out = a (op) b in units of 2^-104 / 2^-205, and its index"""
    mp.mp.prec = PREC
    eps = mp.mpf(2) ** -EPS_BITS[comps]
    worst, at = mp.mpf(0), -1
    for i in range(len(a)):
        x, y = val(a[i]), val(b[i])
        want, got = reference(op, x, y), val(out[i])
        scale = max(abs(x), abs(y)) if op < 2 else abs(want)
        err = abs(got - want) / scale if scale != 0 else abs(got - want)
        if err > worst:
            worst, at = err, i
    return worst / eps, at


def nint_exact(v):
    """libqd's nint: to nearest, halves go up"""
    return mp.floor(v + mp.mpf(1) / 2)


def rnd_we_reference(x, x0, e):
    """FP_NR::rnd_we (nr_FP_dd.inl:234-241): exponent() is ilogb of the leading component + 1"""
    expo = int(np.frexp(x0)[1]) if x0 != 0 else -(1 << 31) + 1   # frexp: x0 = m 2^ex, 1/2 <= |m| < 1: ex = ilogb + 1
    if expo + e >= 53:
        return x
    return nint_exact(x * mp.mpf(2) ** e) / mp.mpf(2) ** e


def normalisation(out, comps):
    """The invariant every result has to keep (the weak libqd form): no zero component followed by a non-zero one, and
    |x[k+1]| <= ulp(x[k]).  Returns (violations, how many components exceed HALF an ulp — allowed, counted)."""
    out = np.asarray(out, dtype=np.float64)[:, :comps]
    bad, above_half = [], 0
    for k in range(comps - 1):
        hi, lo = np.abs(out[:, k]), np.abs(out[:, k + 1])
        ulp = np.spacing(hi)
        viol = ((hi == 0) & (lo != 0)) | ((hi != 0) & (lo > ulp))
        bad += [(int(i), k) for i in np.nonzero(viol)[0]]
        above_half += int(np.count_nonzero((hi != 0) & (lo > ulp / 2)))
    return bad, above_half


# ---- the exact R-factor ------------------------------------------------------------------------------------------
def cholesky_rfactor(b, prec=700):
    """The Householder R-factor of the integer basis b (rows b_i = sum_j R[i][j] q_j, R lower triangular with a
    positive diagonal) is the lower Cholesky factor of the exact integer Gram matrix b b^T.  Computed in mpmath at
    `prec` bits; returns the rows R[i][0..i] as lists of mpf."""
    old = mp.mp.prec
    mp.mp.prec = prec
    try:
        rows = [[int(x) for x in row] for row in b]
        d = len(rows)
        g = [[sum(x * y for x, y in zip(rows[i], rows[j])) for j in range(i + 1)] for i in range(d)]
        L = []
        for i in range(d):
            Li = []
            for j in range(i):
                s = mp.mpf(g[i][j]) - mp.fsum(Li[k] * L[j][k] for k in range(j))
                Li.append(s / L[j][j])
            Li.append(mp.sqrt(mp.mpf(g[i][i]) - mp.fsum(t * t for t in Li)))
            L.append(Li)
        return L
    finally:
        mp.mp.prec = old


# ---- the checks, as data: the host test and the device test run the same list -----------------------------------------
def checks(comps, seed=2024, n=2048):
    """Yields (label, op, a, b, verify) for every element-wise operation: run `op` on the planes a, b (by the host
    harness or on the device) and call verify(out); it asserts the gates of that operation — the mpmath comparison and
    the normalisation invariant — and returns a one-line summary."""
    def normal(label, out):
        bad, above = normalisation(out, comps)
        assert not bad, (comps, label, "not normalised", bad[:4], [list(out[i]) for i, _ in bad[:4]])
        return above

    for op, (name, tol) in ARITH.items():
        a, b, cls = arith_cases(seed, comps, n, "mul" if op in (2, 6) else "add")
        a, b = a.copy(), b.copy()
        if op == 4:
            neg = a[:, 0] < 0
            a[neg] = -a[neg]
        if op == 6:
            b[:, 1:] = 0

        def verify(out, op=op, name=name, tol=tol, a=a, b=b, cls=cls):
            worst, at = arith_error(comps, op, a, b, out)
            assert worst <= tol, (comps, name, "error %s units of 2^-%d" % (mp.nstr(worst, 5), EPS_BITS[comps]),
                                  cls[at], list(a[at]), list(b[at]), list(out[at]))
            above = normal(name, out)
            return "%s: worst error %s of %d units of 2^-%d (class %s); %d components above half an ulp" % (
                name, mp.nstr(worst, 3), tol, EPS_BITS[comps], cls[at], above)
        yield name, op, a, b, verify

    q = nint_cases(seed + 10, comps, n)

    def verify_nint(out, q=q):
        mp.mp.prec = PREC
        for i in range(len(q)):
            x, got = val(q[i]), val(out[i])
            assert got == nint_exact(x), (comps, "nint", list(q[i]), list(out[i]))
        normal("nint", out)
        return "nint: exact on %d operands" % len(q)
    yield "nint", 5, q, q, verify_nint

    a, b, cls = cmp_cases(seed + 20, comps, n)
    for op, name in ((7, "le"), (8, "gt")):
        def verify_cmp(out, op=op, name=name, a=a, b=b, cls=cls):
            mp.mp.prec = PREC
            for i in range(len(a)):
                x, y = val(a[i]), val(b[i])
                want = (x <= y) if op == 7 else (x > y)
                assert list(out[i]) == [1.0 if want else 0.0, 0.0, 0.0, 0.0], (comps, name, cls[i], list(a[i]), list(b[i]))
            return "%s: equals the exact comparison on %d pairs" % (name, len(a))
        yield name, op, a, b, verify_cmp

    a, e, cls = rnd_we_cases(seed + 30, comps, n)

    def verify_rnd(out, a=a, e=e, cls=cls):
        mp.mp.prec = PREC
        kept = 0
        for i in range(len(a)):
            x = val(a[i])
            want = rnd_we_reference(x, float(a[i, 0]), int(e[i, 0]))
            kept += want == x and int(np.frexp(a[i, 0])[1]) + int(e[i, 0]) >= 53
            assert val(out[i]) == want, (comps, "rnd_we", cls[i], list(a[i]), int(e[i, 0]), list(out[i]))
        # (an operand beyond 53 bits comes back as it is: a "gap" operand then keeps its gap — the invariant is about
        # computed results)
        normal("rnd_we", out[[i for i in range(len(a)) if not (cls[i] == "gap" and np.array_equal(out[i], a[i]))]])
        return "rnd_we: exact on %d operands (%d beyond 53 bits, returned as they are)" % (len(a), kept)
    yield "rnd_we", 9, a, e, verify_rnd


def exact_gso(b):
    """The Gram-Schmidt coefficients of the integer basis b in exact rational arithmetic (fractions): (mu, r) with
    r[i][j] = <b_i, b*_j> for j <= i and mu[i][j] = r[i][j] / r[j][j] for j < i — the recurrence of
    MatGSOInterface::update_gso_row on the exact integer Gram matrix."""
    from fractions import Fraction
    rows = [[int(x) for x in row] for row in b]
    d = len(rows)
    g = [[sum(x * y for x, y in zip(rows[i], rows[j])) for j in range(i + 1)] for i in range(d)]
    mu = [[None] * i for i in range(d)]
    r = [[None] * (i + 1) for i in range(d)]
    for i in range(d):
        for j in range(i + 1):
            r[i][j] = Fraction(g[i][j]) - sum((mu[j][k] * r[i][k] for k in range(j)), Fraction(0))
            if j < i:
                mu[i][j] = r[i][j] / r[j][j]
    return mu, r
