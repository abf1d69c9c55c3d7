"""Lists of short / near vectors on the GPU (fplll_amd.svp, fphip_list_vectors): the vector kernel
(list_vectors.hip) against Python big-integer arithmetic, and the solver entry points against known theta series and a
brute-force CPU enumeration."""
import numpy as np
import pytest

import cvp_solver_cases as S
import list_helpers as H

pytestmark = pytest.mark.gpu

BATCHES = [1, 63, 64, 65, 130]  # a partial wave, a full one, more than one
_state = {}


def _case(ctx, which):
    """(g, b) on the 40-row fixture of the closest-vector solver tests / a 72 x 72 basis; open for the module."""
    from fplll_amd.gso import MatGSOBatch
    if which not in _state:
        if which == "q40":
            b = S.basis_of(dict(S.solver_fixtures())["cvpsolve_q40.json"])
        else:
            rng = np.random.default_rng(172)
            b = 1000 * np.eye(72, dtype=np.int64) + rng.integers(-20, 21, size=(72, 72))
        g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
        g.set_basis(b)
        _state[which] = (g, b)
    return _state[which]


def _big(coef, b, target):
    """(vectors, norms) in Python integers."""
    v = coef.astype(object).dot(b.astype(object))
    if target is not None:
        v = v - target.astype(object)[None, :]
    return v, np.array([sum(int(u) * int(u) for u in row) for row in v], dtype=object)


@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("m", BATCHES)
@pytest.mark.parametrize("which", ["q40", "q72"])
def test_vector_kernel_is_big_integer_arithmetic(ctx, which, m, with_target):
    g, b = _case(ctx, which)
    rng = np.random.default_rng(m)
    coef = rng.integers(-2**8, 2**8 + 1, size=(m, b.shape[0]))
    coef[rng.random(coef.shape) < 0.3] = 0
    target = rng.integers(-2**24, 2**24, size=b.shape[1]) if with_target else None
    vec, norm, st = g.records_to_vectors(coef, target)
    want_v, want_n = _big(coef, b, target)
    assert np.all(st == 1)
    assert (vec.astype(object) == want_v).all() and (norm.astype(object) == want_n).all()


def test_one_overflowing_lane_spares_its_neighbours(ctx):
    g, b = _case(ctx, "q40")
    rng = np.random.default_rng(9)
    coef = rng.integers(-8, 9, size=(130, 40))
    coef[40] = 0
    coef[40, 39] = 2**62  # times any entry of row 39 beyond 1: past 2^63
    assert np.abs(b[39]).max() >= 2
    coef[77] = 0
    coef[77, 0] = 2**33  # the vector fits, its squared norm does not
    assert 2 ** 66 * sum(int(v) ** 2 for v in b[0]) >= 2 ** 63 > 2 ** 33 * int(np.abs(b[0]).max())
    vec, norm, st = g.records_to_vectors(coef)
    want_v, want_n = _big(coef, b, None)
    keep = [k for k in range(130) if k not in (40, 77)]
    assert st[40] == -2 and st[77] == -2 and np.all(st[keep] == 1)
    assert not vec[40].any() and norm[40] == 0 and not vec[77].any() and norm[77] == 0
    assert (vec[keep].astype(object) == want_v[keep]).all() and (norm[keep].astype(object) == want_n[keep]).all()


def test_exact_ties_at_the_bound_e8_and_d4(ctx):
    """A bound of EXACTLY the minimum: every minimal vector's norm equals it — the case the integer filter is for."""
    from fplll_amd.svp import short_vectors
    B, scale = H.e8_basis()
    count, coef, vec, norm = short_vectors(ctx, B, 2 * scale)
    assert count == 120 and len(norm) == 120 and np.all(norm == 2 * scale)
    assert (coef.astype(object).dot(np.array(B, dtype=object)) == vec.astype(object)).all()
    assert short_vectors(ctx, B, 2 * scale - 1)[0] == 0
    count, coef, vec, norm = short_vectors(ctx, H.d4_basis(), 2)
    assert count == 12 and np.all(norm == 2)
    assert len({tuple(r) for r in vec.tolist()} | {tuple(-r) for r in vec}) == 24


def test_theta_series(ctx):
    from fplll_amd.svp import theta_series
    with open(H.LEECH_FILE) as fh:
        v = [int(t) for t in fh.read().replace("[", " ").replace("]", " ").split()]
    leech = np.array(v, dtype=np.int64).reshape(24, 24)
    assert theta_series(ctx, leech, 32) == {32: 196560}
    assert theta_series(ctx, H.z8_basis(), 4) == {1: 16, 2: 112, 3: 448, 4: 1136}


def _gs_coords(b, t):
    """(mu, rd, target coordinates) in double: get_gscoords on the GSO of the exact Gram matrix."""
    mu, r = S.gso_double(b)
    mu, rd = S.true_values(mu, r, None)
    d = b.shape[0]
    c = np.zeros(d)
    for i in range(d):
        acc = float(sum(int(u) * int(w) for u, w in zip(t, b[i])))
        for j in range(i):
            acc -= mu[i, j] * c[j]
        c[i] = acc
    return mu, rd, c / rd


def test_vectors_near_on_the_q_ary_fixture(ctx):
    """cvpsolve_q24: with bound_sq = the closest distance of the reference's answer (301), that vector alone; with a
    larger bound — 3600: the lattice's minimum is about 2800, anything below 3000 still holds the one vector — the
    list (221 vectors) of a brute-force CPU enumeration filtered on the exact integer norm."""
    from fplll_amd.svp import vectors_near
    fx = dict(S.solver_fixtures())["cvpsolve_q24.json"]
    b = S.basis_of(fx)
    k = [t["kind"] for t in fx["targets"]].index("near:6")
    t = S.targets_of(fx)[k]
    sol = np.array([int(v) for v in fx["targets"][k]["sol_coord"]], dtype=object)
    w = sol.dot(b.astype(object)) - t.astype(object)
    d0 = sum(int(v) ** 2 for v in w)
    count, coef, vec, norm = vectors_near(ctx, b, t, d0, reduce=False)
    assert count == 1 and [int(v) for v in coef[0]] == [int(v) for v in sol] and int(norm[0]) == d0
    assert [int(v) for v in vec[0]] == [int(v) for v in w]
    bound = 3600
    mu, rd, tc = _gs_coords(b, t)
    brute = S.enumerate_cvp(mu, rd, tc, bound * (1.0 + 2.0 ** -20))
    want = []
    for _, x in brute:
        c = np.array([int(v) for v in x], dtype=object)
        v = c.dot(b.astype(object)) - t.astype(object)
        n2 = sum(int(u) ** 2 for u in v)
        if n2 <= bound:
            want.append((n2, tuple(int(u) for u in c[::-1])))
    count, coef, vec, norm = vectors_near(ctx, b, t, bound, reduce=False)
    got = [(int(n2), tuple(int(u) for u in c[::-1])) for n2, c in zip(norm, coef)]
    print("vectors within 3600 of the target:", count)
    assert count == len(want) >= 100 and got == sorted(want)


def test_reduce_true_gives_the_same_vectors_on_a_reduced_basis(ctx):
    from fplll_amd.svp import short_vectors
    fx = dict(S.solver_fixtures())["cvpsolve_q24.json"]
    b = S.basis_of(fx)
    bound = (3 * sum(int(v) ** 2 for v in b[0])) // 2  # (holds b_0 itself)
    c1, coef1, vec1, norm1 = short_vectors(ctx, b, bound, reduce=False)
    c2, coef2, vec2, norm2 = short_vectors(ctx, b, bound, reduce=True)
    assert c1 == c2 >= 1

    def pm(vec):  # (a reduction may flip which of +-v the half tree holds)
        return sorted(max(tuple(int(u) for u in r), tuple(-int(u) for u in r)) for r in vec)
    assert pm(vec1) == pm(vec2)
    bo = b.astype(object)
    assert (coef1.astype(object).dot(bo) == vec1.astype(object)).all()
    assert (np.asarray(coef2).astype(object).dot(bo) == vec2.astype(object)).all()
