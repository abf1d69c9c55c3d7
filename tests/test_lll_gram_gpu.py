"""Quadratic-form LLL on the GPU (fplll_amd/csrc/lll_gram.hip, fphip_gram_*): every fixture tests/golden/lllgram_*
recorded from the reference — reduced form, u, status, final kappa / swaps / zeros, and mu / r of fphip_gram_update bit
for bit —, seeded random batches against the model of tests/gram_lll_model.py entry by entry, the int64 -> double
rounding above 2^53, the refusals, and the runs with and without u and twice on one handle."""
import numpy as np
import pytest

import gram_lll_model as M
import lll_gram_cases as S

pytestmark = pytest.mark.gpu

NAMES = S.fixture_names()


@pytest.mark.parametrize("name", NAMES)
def test_device_matches_the_reference(ctx, name):
    from fplll_amd.gram import MatGSOGramBatch
    f = S.fixture(name)
    m = MatGSOGramBatch(ctx, np.array(f["G_in"], dtype=np.int64))
    m.enable_transform()
    st, info = m.lll(f["delta"], f["eta"], f["flags"])
    assert int(st[0]) == M.FROM_REF_STATUS[f["status"]]
    assert [int(v) for v in info[0][:3]] == [f["final_kappa"], f["n_swaps"], f["zeros"]]
    assert np.array_equal(m.gram()[0], np.array(f["G_out"], dtype=np.int64))
    assert np.array_equal(m.get_transform()[0], np.array(f["u"], dtype=np.int64))
    # mu and r of fphip_gram_update (fphip_gram_lll ends with one; a second, explicit one gives the same)
    rows = f["gso_rows"]
    for again in (False, True):
        if again:
            ust = m.update()
            assert int(ust[0]) == (1 if rows == f["d"] else 0)
        assert S.same_gso(f, m.mu[0], m.r[0]), "mu / r differ"
    if rows == f["d"]:
        delta = f["delta"] - f["eta"] * f["eta"] if f["flags"] & M.LLL_SIEGEL else f["delta"]
        assert m.is_lll_reduced(0, delta, f["eta"])
    m.close()


def _check_batch_against_model(ctx, forms):
    from fplll_amd.gram import MatGSOGramBatch
    m = MatGSOGramBatch(ctx, forms)
    m.enable_transform()
    st, info = m.lll()
    g, u, mu, r = m.gram(), m.get_transform(), m.mu, m.r
    m.close()
    assert len({forms[k].tobytes() for k in range(len(forms))}) == len(forms)  # different inputs per entry
    for k in range(len(forms)):
        w = M.lll(forms[k].tolist())
        assert w["max_abs"] <= 2**62
        assert int(st[k]) == w["status"], k
        assert [int(v) for v in info[k]] == [w["final_kappa"], w["n_swaps"], w["zeros"], w["iterations"]], k
        assert g[k].tolist() == w["g"], k
        assert u[k].tolist() == w["u"], k
        wmu, wr, rows = M.update_gso(w["g"])
        assert rows == forms.shape[1]
        assert S.tri_equal(wmu, mu[k], strict=True) and S.tri_equal(wr, r[k], strict=False), k


def test_batch_of_64_random_forms_d24(ctx):
    _check_batch_against_model(ctx, S.random_forms(64, 24, 12, seed=2401))


@pytest.mark.parametrize("d", [65, 129])
def test_batch_of_8_lightly_unreduced(ctx, d):
    _check_batch_against_model(ctx, S.lightly_unreduced_forms(8, d, seed=1000 + d))


def test_update_rounds_entries_above_2_53_like_the_host(ctx):
    """get_gram is (double) g(i, j): entries whose low bits do not fit a double, round-to-nearest-even ties included"""
    from fplll_amd.gram import MatGSOGramBatch
    rng = np.random.default_rng(53)
    d = 6
    g = np.zeros((d, d), dtype=np.int64)
    for i in range(d):
        for j in range(i):
            g[i, j] = g[j, i] = int(rng.integers(-(1 << 56), 1 << 56)) | 1
        g[i, i] = (1 << 60) + (1 << 58) * i + int(rng.integers(0, 1 << 20)) * 2 + 1
    g[1, 0] = g[0, 1] = (1 << 54) + 2          # a tie: halfway between two doubles, rounds to the even one
    g[2, 0] = g[0, 2] = -((1 << 54) + 6)       # a tie the other way
    g[3, 1] = g[1, 3] = (1 << 55) + 3          # not a tie
    assert any(int(float(int(x))) != int(x) for x in g.ravel())
    m = MatGSOGramBatch(ctx, g)
    m.update()
    mu, r, _ = M.update_gso(g.tolist())
    assert S.tri_equal([row[:i] for i, row in enumerate(mu)], m.mu[0], strict=True)
    assert S.tri_equal([row[:i + 1] for i, row in enumerate(r)], m.r[0], strict=False)
    m.close()


def test_refusals(ctx):
    from fplll_amd import _lib
    from fplll_amd.gram import MatGSOGramBatch
    import ctypes
    g = S.random_forms(2, 5, 6, seed=5)
    m = MatGSOGramBatch(ctx, g)
    before = m.gram()
    bad = g.copy()
    bad[1, 3, 1] += 1
    with pytest.raises(_lib.HipError, match="not symmetric"):
        m.set_gram(bad)
    assert np.array_equal(m.gram(), before)  # nothing was uploaded
    assert "form 1" in ctx.last_error()
    m.close()
    h = ctypes.c_void_p()
    assert ctx.lib.fphip_gram_create(ctx.handle, 1, 257, ctypes.byref(h)) == _lib.FPHIP_UNSUPPORTED
    assert not h.value
    with pytest.raises(NotImplementedError):
        MatGSOGramBatch(ctx, np.eye(257, dtype=np.int64))


def test_without_the_transform_and_twice_on_one_handle(ctx):
    from fplll_amd.gram import MatGSOGramBatch
    forms = S.random_forms(5, 20, 10, seed=77)
    a = MatGSOGramBatch(ctx, forms)
    st_a, info_a = a.lll()
    g_a = a.gram()
    b = MatGSOGramBatch(ctx, forms)
    b.enable_transform()
    st_b, info_b = b.lll()
    g_b, u_b, mu_b, r_b = b.gram(), b.get_transform(), b.mu, b.r
    assert np.array_equal(st_a, st_b) and np.array_equal(info_a, info_b) and np.array_equal(g_a, g_b)
    assert list(st_b) == [1] * 5 and not np.array_equal(g_b, forms)
    # the same handle again on the same input
    b.set_gram(forms)
    st_c, info_c = b.lll()
    assert np.array_equal(st_c, st_b) and np.array_equal(info_c, info_b)
    assert np.array_equal(b.gram(), g_b) and np.array_equal(b.get_transform(), u_b)
    assert b.mu.tobytes() == mu_b.tobytes() and b.r.tobytes() == r_b.tobytes()
    a.close()
    b.close()


def test_lll_reduction_gram_one_form_and_a_batch(ctx):
    from fplll_amd import lll_reduction_gram
    forms = S.random_forms(3, 12, 8, seed=12)
    g1, u1, st1 = lll_reduction_gram(ctx, forms[0])
    assert st1 == 1 and g1.shape == (12, 12)
    uo = u1.astype(object)
    assert (uo.dot(forms[0].astype(object)).dot(uo.T) == g1.astype(object)).all()
    gb, ub, stb = lll_reduction_gram(ctx, forms, with_u=False)
    assert ub is None and list(stb) == [1, 1, 1] and np.array_equal(gb[0], g1)
