"""The closest-vector solver on the GPU: the target preparation kernel and MatGSOBatch.babai against their Python
restatements (tests/cvp_solver_cases.py, bit for bit, fed with the device's own mu / r / row exponents), and
fplll_amd.cvp.closest_vector(s) against the reference's answers — the five known-answer cases of its test suite
(tests/golden/kat_cvp.json) and closest_vector runs of the reference itself (tests/golden/cvpsolve_*.json)."""
import numpy as np
import pytest

import cvp_solver_cases as S

pytestmark = pytest.mark.gpu

FIXTURES = dict(S.solver_fixtures())
BATCHES = [1, 63, 64, 65, 130]  # a partial wave, a full one, more than one
_state = {}


def _targets_around(b, seed, count, far_every=9):
    """`count` integer targets around the lattice of b: lattice points with coefficients in [-8, 8] (every
    `far_every`-th: around 2^30) plus offsets in [-6, 6]; exact Python integers brought to int64."""
    rng = np.random.default_rng(seed)
    d, n = b.shape
    out = []
    for k in range(count):
        span = 2**30 if k % far_every == far_every - 1 else 8
        c = rng.integers(-span, span + 1, size=d)
        t = c.astype(object).dot(b.astype(object)) + rng.integers(-6, 7, size=n).astype(object)
        out.append([int(v) for v in t])
    return np.array(out, dtype=np.int64)


def _case(ctx, which):
    """(g, b, targets [130][n], restatement of all 130) on the d = 40 solver fixture / a 72 x 72 basis; the object
    stays open for the module (closed with the context)."""
    from fplll_amd.gso import MatGSOBatch, lll_reduction
    if which not in _state:
        if which == "q40":
            b = S.basis_of(FIXTURES["cvpsolve_q40.json"])
            fixed = S.targets_of(FIXTURES["cvpsolve_q40.json"])
        else:  # 72 x 72: a seeded q-ary basis, reduced on the device
            rng = np.random.default_rng(72)
            b = np.zeros((72, 72), dtype=np.int64)
            b[:36, :36] = np.eye(36, dtype=np.int64)
            b[:36, 36:] = rng.integers(0, 2039, size=(36, 36))
            b[36:, 36:] = 2039 * np.eye(36, dtype=np.int64)
            b, _, status, _ = lll_reduction(ctx, b, with_u=False)
            assert status == 1
            fixed = np.zeros((0, 72), dtype=np.int64)
        tg = np.concatenate([fixed, _targets_around(b, 7, 130 - len(fixed))])
        g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
        g.set_basis(b)
        assert g.update_gso()[0] == 1
        mu, rd = S.true_values(g.get_mu_matrix(0), g.get_r_matrix(0), g.row_expo(0))
        _state[which] = (g, b, tg, mu, rd, S.prepare(b, mu, rd, tg))
    return _state[which]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("T", BATCHES)
@pytest.mark.parametrize("which", ["q40", "q72"])
def test_preparation_is_the_restatement_bit_for_bit(ctx, which, T):
    g, b, tg, mu, rd, P = _case(ctx, which)
    coef, tc, desc, st = g.cvp_prepare(tg[:T])
    assert list(st) == list(P["status"][:T]) and np.all(st == 1)
    assert np.array_equal(coef, P["coef"][:T])
    assert _same_bits(tc, P["target_coord"][:T])
    assert _same_bits(desc, P["descent"][:T])


def test_far_targets_take_more_than_one_pass(ctx):
    """The targets with entries around 2^40 are reduced by a first pass (non-zero coefficients: the subtraction ran,
    so a second pass checked the result), and the restatement — which the kernel equals — counts the passes."""
    g, b, tg, mu, rd, P = _case(ctx, "q40")
    far = [k for k in range(len(tg)) if np.abs(tg[k]).max() > 2**36]
    assert len(far) >= 10
    coef, _, _, st = g.cvp_prepare(tg)
    for k in far:
        assert P["passes"][k] >= 2 and st[k] == 1 and np.any(coef[k] != 0)


def test_overflowing_target_gives_minus_two_and_spares_the_others(ctx):
    from fplll_amd.gso import MatGSOBatch
    b, mu_r, rd_r, tg = S.overflow_case()
    g = MatGSOBatch(ctx, 1, 2, 2)
    try:
        g.set_basis(b)
        assert g.update_gso()[0] == 1
        mu, rd = S.true_values(g.get_mu_matrix(0), g.get_r_matrix(0), g.row_expo(0))
        P = S.prepare(b, mu, rd, tg)
        coef, tc, desc, st = g.cvp_prepare(tg)
        assert list(st) == [-2, 1, 1] == list(P["status"])
        assert np.array_equal(coef, P["coef"]) and _same_bits(tc, P["target_coord"]) and _same_bits(desc, P["descent"])
        assert not coef[0].any() and list(coef[1]) == [5 - 7 * 2**20, 7]
    finally:
        g.close()
    # in a wave of its own targets: lane 40 of 130 overflows (an entry beyond what the products allow), the others
    # keep the results they have without it
    g, b, tg, mu, rd, P = _case(ctx, "q40")
    bad = tg.copy()
    bad[40] = 2**62
    Pb = S.prepare(b, mu, rd, bad[40:41])
    coef, tc, desc, st = g.cvp_prepare(bad)
    assert st[40] == Pb["status"][0] == -2
    keep = [k for k in range(len(tg)) if k != 40]
    assert np.all(st[keep] == 1) and np.array_equal(coef[keep], P["coef"][keep])
    assert _same_bits(tc[keep], P["target_coord"][keep]) and _same_bits(desc[keep], P["descent"][keep])


@pytest.mark.parametrize("which", ["q40", "q72"])
def test_babai_is_the_restatement(ctx, which):
    """MatGSOBatch.babai: float coordinates, the integer overload, and a start / dimension sub-range."""
    g, b, tg, mu, rd, P = _case(ctx, which)
    d = b.shape[0]
    rng = np.random.default_rng(11)
    v = rng.uniform(-1000, 1000, size=(130, d))
    v[3, d - 1] = 2.5  # a tie: rint goes to the even neighbour
    w, st = g.babai(v)
    wr, sr = S.babai(mu, v)
    assert np.array_equal(w, wr) and list(st) == list(sr) and w[3, d - 1] == 2
    vi = rng.integers(-1000, 1000, size=(65, d))
    w, st = g.babai(vi)
    wr, _ = S.babai(mu, vi.astype(np.float64))
    assert np.array_equal(w, wr)
    start, dim = 5, d - 12
    w, st = g.babai(v[:, :dim], start=start, dimension=dim)
    wr, _ = S.babai(mu, v[:, :dim], start=start, dimension=dim)
    assert w.shape == (130, dim) and np.array_equal(w, wr)
    w1, s1 = g.babai(v[0])
    assert np.array_equal(w1, S.babai(mu, v[:1])[0][0]) and s1 == 1
    big = np.zeros((2, d))
    big[0, d - 1] = 1e30
    w, st = g.babai(big)
    assert list(st) == [-2, 1] and not w.any()


def test_known_answer_cases(ctx):
    """The reference's own test (tests/test_cvp.cpp): LLL-reduce, solve, multiply back — the expected vectors exactly."""
    from fplll_amd.cvp import closest_vector
    for c in S.load("kat_cvp.json")["cases"]:
        sol, vec = closest_vector(ctx, c["basis"], c["target"], reduce=True)
        assert [int(v) for v in vec] == c["expected"], c["name"]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_reference_sol_coord_single_and_batch(ctx, name):
    """Every recorded target: the reference's sol_coord exactly — one call per target, and one call for all of them."""
    from fplll_amd.cvp import closest_vector, closest_vectors
    fx = FIXTURES[name]
    b, tg = S.basis_of(fx), S.targets_of(fx)
    want = [[int(v) for v in t["sol_coord"]] for t in fx["targets"]]
    sols, vecs, dists = closest_vectors(ctx, b, tg, with_dist=True)
    assert [[int(v) for v in s] for s in sols] == want
    for k, t in enumerate(fx["targets"]):
        sol, vec = closest_vector(ctx, b, tg[k])
        assert [int(v) for v in sol] == want[k], t["kind"]
        assert [int(v) for v in vec] == [int(v) for v in vecs[k]]
        diff = np.array([int(v) for v in vec], dtype=object) - tg[k].astype(object)
        assert abs(float(sum(int(v) ** 2 for v in diff)) - dists[k]) <= 1e-9 * max(1.0, dists[k])
        if t["kind"] == "lattice":  # the lattice point returns itself, at distance exactly 0
            assert [int(v) for v in vec] == [int(v) for v in tg[k]] and dists[k] == 0.0


def test_solver_above_64_rows_finds_the_planted_points(ctx, monkeypatch):
    """72 x 72, nearly orthogonal (1000 on the diagonal, entries in [-20, 20] elsewhere: LLL-reduced as it stands,
    shortest vectors of length about 1000): targets = lattice points with known coefficients (every fourth around
    2^30) plus offsets in [-40, 40] — a norm of about 200, far below half the minimum, so the planted point is the
    closest.  The solver returns its coefficients; it asks the enumerator for blocks above 64 rows itself (no switch
    set), and the coefficients of the levels >= 64 come back through the top walk."""
    from fplll_amd.cvp import closest_vectors
    monkeypatch.delenv("FPHIP_CVP_WIDE", raising=False)
    rng = np.random.default_rng(172)
    b = 1000 * np.eye(72, dtype=np.int64) + rng.integers(-20, 21, size=(72, 72))
    want = np.array([rng.integers(-(2**30 if k % 4 == 3 else 8), (2**30 if k % 4 == 3 else 8) + 1, size=72)
                     for k in range(8)])
    off = rng.integers(-40, 41, size=(8, 72))
    tg = (want.astype(object).dot(b.astype(object)) + off.astype(object)).astype(np.int64)
    sol, vec, dist = closest_vectors(ctx, b, tg, with_dist=True)
    assert np.array_equal(sol, want)
    assert [float(v) for v in (off.astype(object) ** 2).sum(axis=1)] == pytest.approx(list(dist), rel=1e-9)


def test_a_second_enumeration_context(ctx):
    """ectx: the enumerations run on a context of their own; the same answers."""
    import fplll_amd
    from fplll_amd.cvp import closest_vectors
    fx = FIXTURES["cvpsolve_q36.json"]
    e2 = fplll_amd.Context(0)
    try:
        sols, _ = closest_vectors(ctx, S.basis_of(fx), S.targets_of(fx), ectx=e2)
    finally:
        e2.close()
    assert [[int(v) for v in s] for s in sols] == [[int(v) for v in t["sol_coord"]] for t in fx["targets"]]


def test_proved_method_is_declined(ctx):
    from fplll_amd.cvp import CVPM_PROVED, closest_vector
    from fplll_amd.enumeration import Unsupported
    fx = FIXTURES["cvpsolve_q24.json"]
    with pytest.raises(Unsupported, match="CVPM_PROVED.*CVPM_FAST only"):
        closest_vector(ctx, S.basis_of(fx), S.targets_of(fx)[0], method=CVPM_PROVED)
    with pytest.raises(Unsupported, match="CVPM_FAST only"):
        closest_vector(ctx, S.basis_of(fx), S.targets_of(fx)[0], method=1)
