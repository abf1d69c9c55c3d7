"""The closest-vector solver (fplll_amd.cvp, fphip_closest_vector, fphip_cvp_prepare, MatGSOBatch.babai), the CPU half:
the conditions of its fixtures, the Python restatement of the preparation kernel (tests/cvp_solver_cases.py) against
mpmath at 200 bits, and the C ABI's view of the new exports.  No GPU.

Fixtures: tests/golden/kat_cvp.json (the reference's five known-answer cases) and tests/golden/cvpsolve_q{24,36,40}.json
(lll_reduction + closest_vector of the reference itself on seeded q-ary bases: tests/native/closest_vector_ref_driver.cpp,
tests/golden/make_cvp_solver_fixtures.sh)."""
import ctypes
import os

import numpy as np
import pytest

import conftest as C
import cvp_solver_cases as S

FIXTURES = S.solver_fixtures()
_prep_cache = {}


def _prepared(name):
    """(b, targets, true mu, true r_ii, prepare(...)) of a fixture on a double GSO of its basis, computed once."""
    if name not in _prep_cache:
        fx = dict(FIXTURES)[name]
        b, tg = S.basis_of(fx), S.targets_of(fx)
        mu, rd = S.true_values(*S.gso_double(b), None)
        _prep_cache[name] = (b, tg, mu, rd, S.prepare(b, mu, rd, tg))
    return _prep_cache[name]


def test_fixture_set():
    assert [n for n, _ in FIXTURES] == ["cvpsolve_q24.json", "cvpsolve_q36.json", "cvpsolve_q40.json"]
    assert [fx["d"] for _, fx in FIXTURES] == [24, 36, 40]
    for _, fx in FIXTURES:
        kinds = [t["kind"].split(":")[0] for t in fx["targets"]]
        assert len(kinds) >= 4 and "lattice" in kinds and "far" in kinds
        assert all(t["status"] == 0 for t in fx["targets"])  # fplll's RED_SUCCESS
        far = [t for t in fx["targets"] if t["kind"].startswith("far")][0]
        assert max(abs(v) for v in far["target"]) > 2**36  # entries around 2^40


def test_known_answer_cases_are_the_references():
    kat = S.load("kat_cvp.json")
    assert [(c["d"], c["n"]) for c in kat["cases"]] == [(30, 30), (30, 30), (42, 42), (10, 10), (10, 10)]
    for c in kat["cases"]:
        b = np.array(c["basis"], dtype=object)
        assert b.shape == (c["d"], c["n"]) and abs(b).max() < 2**11
        # the expected vector is a lattice point: exact rational solve of x b = expected
        import fractions
        m = [[fractions.Fraction(int(v)) for v in row] for row in b.T.tolist()]
        rhs = [fractions.Fraction(int(v)) for v in c["expected"]]
        d = c["d"]
        for col in range(d):
            piv = next(i for i in range(col, d) if m[i][col] != 0)
            m[col], m[piv], rhs[col], rhs[piv] = m[piv], m[col], rhs[piv], rhs[col]
            for i in range(d):
                if i != col and m[i][col] != 0:
                    f = m[i][col] / m[col][col]
                    m[i] = [a - f * p for a, p in zip(m[i], m[col])]
                    rhs[i] -= f * rhs[col]
        assert all((rhs[i] / m[i][i]).denominator == 1 for i in range(d)), c["name"]


@pytest.mark.parametrize("name", [n for n, _ in FIXTURES])
def test_every_target_has_one_closest_vector(name):
    """The uniqueness condition: around every target a fixed-radius enumeration at 1.01 times the squared distance of
    the reference's answer holds exactly one candidate — that answer.  (Double restatement on the double GSO; a tied
    instance would have no single right answer.)"""
    fx = dict(FIXTURES)[name]
    b, tg, mu, rd, P = _prepared(name)
    d = len(rd)
    assert np.all(P["status"] == 1)
    for k, t in enumerate(fx["targets"]):
        x = np.array([float(int(s) - int(c)) for s, c in zip(t["sol_coord"], P["coef"][k])])
        c = P["target_coord"][k]
        dist = 0.0
        for i in range(d - 1, -1, -1):
            ci = c[i] - sum(x[j] * mu[j, i] for j in range(i + 1, d))
            dist += (x[i] - ci) ** 2 * rd[i]
        if t["kind"] == "lattice":
            assert dist == 0.0 and P["descent"][k] == 0.0
            assert list(np.array(t["sol_coord"], dtype=object).dot(b.astype(object))) == t["target"]
            continue
        assert dist > 0.0 and P["descent"][k] >= dist * (1 - 1e-9)
        cands = S.enumerate_cvp(mu, rd, c, 1.01 * dist)
        assert len(cands) == 1 and cands[0][1] == tuple(x), (t["kind"], len(cands))


@pytest.mark.parametrize("name", [n for n, _ in FIXTURES])
def test_restatement_rounds_like_200_bits(name):
    """The double restatement of the preparation and the same loop in mpmath at 200 bits round alike: the same number
    of passes, the same accumulated coefficients, the same rounding descent — and not by luck: no value that is
    rounded lies within 1e-6 of a half-integer.  The far target takes more than one pass."""
    fx = dict(FIXTURES)[name]
    b, tg, mu, rd, P = _prepared(name)
    xd, _ = S.descent_of(mu, rd, P["target_coord"])
    for k, t in enumerate(fx["targets"]):
        m = S.prepare_mp(b, tg[k])
        assert m["margin"] > 1e-6, (t["kind"], m["margin"])
        assert m["passes"] == P["passes"][k]
        assert m["coef"] == [int(v) for v in P["coef"][k]]
        assert m["descent_x"] == [int(v) for v in xd[k]]
        if t["kind"].startswith("far"):
            assert P["passes"][k] >= 2 and any(v != 0 for v in m["coef"])


def test_restatement_statuses():
    """Beyond 63 bits: status -2 for that target alone, its outputs zero; the loop limit: -1."""
    b, mu, rd, tg = S.overflow_case()
    Q = S.prepare(b, mu, rd, tg)
    assert list(Q["status"]) == [-2, 1, 1]
    assert not Q["coef"][0].any() and not Q["target_coord"][0].any() and Q["descent"][0] == 0.0
    assert list(Q["coef"][1]) == [5 - 7 * 2**20, 7] and list(Q["coef"][2]) == [0, 0]
    b, tg, mu, rd, P = _prepared("cvpsolve_q24.json")
    L = S.prepare(b, mu, rd, tg[:2], max_passes=1)  # both need two passes
    assert list(L["status"]) == [-1, -1] and not L["coef"].any() and not L["target_coord"].any()


def test_babai_restatement_is_the_nearest_plane_loop():
    b, tg, mu, rd, P = _prepared("cvpsolve_q24.json")
    d = len(rd)
    rng = np.random.default_rng(5)
    v = rng.uniform(-50, 50, size=(7, d))
    w, st = S.babai(mu, v)
    assert np.all(st == 1)
    # w is an integer vector whose Gram-Schmidt coordinates are within 1/2 (+ rounding) of v's
    for k in range(7):
        c = np.array([w[k, j] + sum(w[k, i] * mu[i, j] for i in range(j + 1, d)) for j in range(d)])
        assert np.all(np.abs(c - v[k]) <= 0.5 + 1e-9)
    ws, _ = S.babai(mu, v[:, :6], start=10, dimension=6)
    assert ws.shape == (7, 6)
    half = np.zeros((1, d))
    half[0, d - 1] = 2.5  # ties to even (FP_NR<double>::rnd is rint)
    assert S.babai(mu, half)[0][0, d - 1] == 2


def test_abi_exports_the_solver(tmp_path):
    """The three new entry points are exported with C linkage and declared in the header; the method constants are
    fplll's (CVPM_FAST = 0, CVPM_PROVED = 2)."""
    import fplll_amd
    from fplll_amd import cvp
    lib = fplll_amd.load()
    for s in ("fphip_cvp_prepare", "fphip_gso_babai", "fphip_closest_vector"):
        assert getattr(lib, s)
    hdr = open(os.path.join(C.ROOT, "include", "fplll_hip.h")).read()
    assert "#define FPHIP_CVPM_FAST 0" in hdr and "#define FPHIP_CVPM_PROVED 2" in hdr
    assert (cvp.CVPM_FAST, cvp.CVPM_PROVED) == (0, 2)
    # without a handle the calls fail cleanly (no device is touched)
    lib.fphip_closest_vector.restype = ctypes.c_int
    lib.fphip_closest_vector.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p, ctypes.c_int] + \
        [ctypes.c_void_p] * 3
    assert lib.fphip_closest_vector(None, None, 0, 1, None, 0, None, None, None) == -1
    for f in ("closest_vector", "closest_vectors"):
        assert callable(getattr(cvp, f))
    from fplll_amd.gso import MatGSOBatch
    assert callable(MatGSOBatch.babai) and callable(MatGSOBatch.cvp_prepare)
