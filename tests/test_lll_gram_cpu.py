"""Quadratic-form LLL, the CPU side: tests/gram_lll_model.py (a plain restatement of MatGSOGram + lll()) reproduces
every fixture tests/golden/lllgram_* recorded from the reference — the reduced form, u, status, the three counters, and
mu / r of the final update_gso bit for bit — and the fixtures satisfy their own conditions (u G_in u^T = G_out in exact
integers, |det u| = 1, G_out symmetric, (u A)(u A)^T = G_out where a basis A is behind the form, the reference's
is_lll_reduced accepts the result, no |entry| of g beyond 2^62 along the run)."""
import math

import numpy as np
import pytest

import gram_lll_model as M
import lll_gram_cases as S

NAMES = S.fixture_names()
# The rank-deficient form: with zero rows the reference's MatGSOGram::move_row rotates u, mu and r to the end of the
# matrix but g only within the rows it has discovered (gso_gram.cpp:334-345: not at all when the zero row is the last
# known one), so the zero row stays where it was, is found again, and lll() ends with zeros = d - 3 = 5 for the row
# that repeats at position 3: g_out and u no longer belong together from that row on.  The model and the device follow
# the reference there (the parity tests); of the conditions below, the ones that relate g_out to u hold on the rows
# above the first zero row only, and that is what is asserted for this one fixture.
RANKDEF = "rankdef"


def test_all_the_cases_are_recorded():
    want = {"example2", "cvp_lattice", "cvp_lattice2", "cvp_lattice3", "cvp_lattice4", "cvp_lattice5", "intrel_40_10",
            "intrel_50_20", "cvp_lattice4_siegel", "cvp_lattice4_early", RANKDEF, "form_nobasis", "d1", "d2", "d3",
            "w64", "w65", "w128", "w129", "w192", "w193", "w256"}
    assert want <= set(NAMES), sorted(want - set(NAMES))
    assert S.fixture(RANKDEF)["zeros"] > 0
    assert S.fixture("cvp_lattice4_siegel")["flags"] == M.LLL_SIEGEL
    assert S.fixture("cvp_lattice4_early")["flags"] == M.LLL_EARLY_RED
    for k in ("G_out", "u", "status", "final_kappa", "n_swaps", "zeros", "mu", "r"):  # LLL_EARLY_RED changes nothing
        assert S.fixture("cvp_lattice4_early")[k] == S.fixture("cvp_lattice4")[k], k
    assert "A" not in S.fixture("form_nobasis")


@pytest.mark.parametrize("name", NAMES)
def test_model_reproduces_the_reference(name):
    f, m = S.fixture(name), S.model_run(name)
    assert m["status"] == M.FROM_REF_STATUS[f["status"]]
    assert (m["final_kappa"], m["n_swaps"], m["zeros"]) == (f["final_kappa"], f["n_swaps"], f["zeros"])
    assert m["g"] == f["G_out"]
    assert m["u"] == f["u"]
    mu, r, rows = S.model_gso(name)
    assert rows == f["gso_rows"]
    assert S.same_gso(f, mu, r), "mu / r differ"
    assert m["max_abs"] <= 2**62, math.log2(m["max_abs"])


def _imat(a):
    return np.array([[int(x) for x in row] for row in a], dtype=object)


def _mul(a, b):
    """Exact product of integer matrices: int64 where the bound allows, Python integers otherwise."""
    amax = max([abs(int(x)) for x in a.ravel()] + [0])
    bmax = max([abs(int(x)) for x in b.ravel()] + [0])
    if a.shape[1] * amax * bmax < 2**62:
        return a.astype(np.int64).dot(b.astype(np.int64)).astype(object)
    return a.dot(b)


def _det_mod(a, p):
    a = np.array(a % p, dtype=np.int64)
    n, det = a.shape[0], 1
    for k in range(n):
        piv = next((i for i in range(k, n) if a[i, k]), None)
        if piv is None:
            return 0
        if piv != k:
            a[[k, piv]] = a[[piv, k]]
            det = -det
        det = det * int(a[k, k]) % p
        inv = pow(int(a[k, k]), p - 2, p)
        fac = a[k + 1:, k] * inv % p
        a[k + 1:, k:] = (a[k + 1:, k:] - fac[:, None] * a[k, k:][None, :] % p) % p
    return det % p


def det_exact(a):
    """det of an integer matrix: modulo enough 31-bit primes to cover Hadamard's bound, then the Chinese remainder."""
    bound = 1
    for row in a:
        bound *= math.isqrt(sum(int(x) * int(x) for x in row)) + 1
    primes, prod, p = [], 1, 2**31 - 1
    while prod <= 2 * bound + 1:
        while any(p % q == 0 for q in range(2, 1 << 8)) or pow(2, p - 1, p) != 1 or pow(3, p - 1, p) != 1:
            p -= 2
        primes.append(p)
        prod *= p
        p -= 2
    x = 0
    for p in primes:
        mi = prod // p
        x = (x + _det_mod(a, p) * mi * pow(mi, -1, p)) % prod
    return x - prod if x > prod // 2 else x


@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    from fplll_amd.gso import is_lll_reduced
    f = S.fixture(name)
    d = f["d"]
    gin, gout, u = _imat(f["G_in"]), _imat(f["G_out"]), _imat(f["u"])
    if "sha256" in f:  # a compact record holds the digests of the reference's own G_in and G_out
        assert S.digest_int(f["G_in"]) == f["sha256"]["G_in"] and S.digest_int(f["G_out"]) == f["sha256"]["G_out"]
    top = d if name != RANKDEF else d - f["zeros"]  # (see RANKDEF above)
    assert (gout == gout.T).all()
    assert abs(det_exact(u)) == 1
    cong = _mul(_mul(u, gin), u.T)
    assert (cong[:top, :top] == gout[:top, :top]).all()
    if "A" in f:
        ua = _mul(u, _imat(f["A"]))
        assert (_mul(ua, ua.T)[:top, :top] == gout[:top, :top]).all()
    # the reference's predicate on mu / r of the result (no row exponents)
    rows = f["gso_rows"]
    assert rows == d or name == RANKDEF
    k = min(top, rows)
    if "sha256" in f:  # mu and r of the recorded g_out: the model's, which carry the reference's digests
        assert S.model_run(name)["g"] == f["G_out"]
        mmu, mr, _ = S.model_gso(name)
        assert S.same_gso(f, mmu, mr)
        mu, r = np.tril(np.array(mmu), -1), np.tril(np.array(mr))
    else:
        mu, r = np.zeros((k, k)), np.zeros((k, k))
        for i in range(k):
            mu[i, :i] = f["mu"][i][:i]
            r[i, :i + 1] = f["r"][i][:i + 1]
    # (LLL_SIEGEL swaps until r(i,i) >= (delta - eta^2) r(i-1,i-1), which gives Lovasz's condition r(i,i) +
    #  mu(i,i-1)^2 r(i-1,i-1) >= delta' r(i-1,i-1) for delta' = delta - eta^2 and no larger one)
    delta = f["delta"] - f["eta"] * f["eta"] if f["flags"] & M.LLL_SIEGEL else f["delta"]
    assert is_lll_reduced(mu, r, np.zeros(k, dtype=np.int64), delta, f["eta"])
    assert max(abs(int(x)) for x in gin.ravel()) <= 2**62 and max(abs(int(x)) for x in gout.ravel()) <= 2**62
