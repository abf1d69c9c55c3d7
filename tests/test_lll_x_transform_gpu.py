"""The transformation matrix u under lll_ex (53 / 106 / 212 bits) and lll_ladder (MatGSOBatch.enable_transform /
fphip_gso_enable_transform): lll_x_u_kernel<NQ, FT>, lll_x_u.hip.

Every case runs the tracked object next to its untracked twin (tests/lll_x_transform_cases.py): tracking changes
nothing of the run, an uploaded u0 is multiplied from the left, and u b_in = b_out in exact integers with |det u| = 1.
The tree-order kernel need not return the reference's basis, so u is held against the basis the DEVICE returns; where
b_in has full row rank (shown first) that fixes u uniquely.  Every comparison of integers is exact.

Not launched here: precision 212 with more than 64 rows or columns, tracked or not (OPEN)."""
import time

import numpy as np
import pytest

import conftest as C
import hlll_transform_cases as T
import lll_x_transform_cases as X
import wide_cases as W

pytestmark = pytest.mark.gpu


def _ex(f, prec):
    return lambda g: g.lll_ex(prec, f["kmin"], f["kstart"], f["kend"], f["delta"], f["eta"])


# ---- 1. full-rank fixtures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [53, 106])
@pytest.mark.parametrize("name", ["lll_q40", "lll_q72", "lll_u24", "lll_r30"])
def test_full_rank_fixture(ctx, name, prec):
    """b_in has independent rows (a minor that is non-singular modulo a prime), so ONE integer matrix takes it to the
    basis the device returns: u is that matrix.  lll_q72: two columns per lane, rows and columns of u in the second
    chunk."""
    f = X.lll_fixture(name)
    assert X.full_row_rank(f["b_in"])
    t = time.time()
    st, info, out, u, _, ms = X.tracked_and_twin(ctx, [f["b_in"]], _ex(f, prec))
    assert list(st) == [1, 1], (st, info)
    assert int(info[0][1]) > 0   # (the run did exchange rows)
    T.check_transform(u[0], f["b_in"], out[0])
    C.note(lambda: ("lll_ex(%d) with u %s: %d swaps, kernel %.1f ms, test %.1f s"
                    % (prec, name, int(info[0][1]), ms, time.time() - t),))


# ---- 2. rank-deficient fixtures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [53, 106])
@pytest.mark.parametrize("name", ["lll_q40_zero2", "lll_q40_dup2", "lll_q40_zero1_dup2_u"])
def test_rank_deficient_fixture(ctx, name, prec):
    """zero and duplicated rows: the zero rows go to the end on the slot table, and the rows of u go with them.  u is
    not determined by the bases there, the relation and the determinant are."""
    f = X.lll_fixture(name)
    st, info, out, u, _, _ = X.tracked_and_twin(ctx, [f["b_in"]], _ex(f, prec))
    assert list(st) == [1, 1], (st, info)
    zeros = f["zeros"]
    assert zeros > 0 and int(info[0][2]) == zeros
    assert not out[0][f["d"] - zeros:].any() and np.all(np.any(out[0][:f["d"] - zeros] != 0, axis=1))
    X.relation(u[0], f["b_in"], out[0])   # (its last rows are therefore integer relations of the rows of b_in)
    if "u_out" in f:
        C.note(lambda: ("%s at %d bits: u %s the reference's u_out, basis %s the reference's"
                        % (name, prec, "==" if np.array_equal(u[0], f["u_out"]) else "!=",
                           "==" if np.array_equal(out[0], f["b_out"]) else "!="),))


# ---- 3. sub-ranges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [53, 106])
@pytest.mark.parametrize("name", ["lll_q40_range10_30", "lll_q40_kmin5"])
def test_sub_range(ctx, name, prec):
    """lll(kappa_min, kappa_start, kappa_end): the rows from kappa_end on are not touched — neither b's nor u's, for
    the identity and for the uploaded u0"""
    f = X.lll_fixture(name)
    kend = f["kend"]
    assert 0 < kend < f["d"]
    st, info, out, u, u0, _ = X.tracked_and_twin(ctx, [f["b_in"]], _ex(f, prec))
    C.note(lambda: ("lll_ex(%d) with u %s: status %s, info %s" % (prec, name, list(st), info.tolist()),))
    assert X.full_row_rank(f["b_in"])
    T.check_transform(u[0], f["b_in"], out[0])   # (whatever the status)
    assert np.array_equal(out[0][kend:], f["b_in"][kend:])
    assert np.array_equal(u[0][kend:], np.eye(f["d"], dtype=np.int64)[kend:])
    assert np.array_equal(u[1][kend:], u0[0][kend:])


# ---- 4. quad-double, one column per lane ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lll_q40", "lll_u24"])
def test_quad_double(ctx, name):
    f = X.lll_fixture(name)
    assert max(f["d"], f["n"]) <= 64
    st, info, out, u, _, ms = X.tracked_and_twin(ctx, [f["b_in"]], _ex(f, 212))
    assert list(st) == [1, 1], (st, info)
    assert np.array_equal(out[0], f["b_out"]) and int(info[0][1]) == f["n_swaps"]   # (as the untracked run, test_dd_gpu.py)
    assert X.full_row_rank(f["b_in"])
    T.check_transform(u[0], f["b_in"], f["b_out"])
    C.note(lambda: ("lll_ex(212) with u %s: %d swaps, kernel %.1f ms" % (name, int(info[0][1]), ms),))


# ---- 5. every columns-per-lane instantiation, double and double-double ----------------------------------------------------------------
WIDE = [("short", d, n) for d, n in W.SHORT_WIDE] + [("tall", 3), ("tall", 4)]


def _wide_id(case):
    return "%dx%d" % case[1:] if case[0] == "short" else "tall%d" % W.tall_base(case[1]).shape[0]


@pytest.mark.parametrize("prec", [53, 106])
@pytest.mark.parametrize("case", WIDE, ids=_wide_id)
def test_every_nq(ctx, case, prec):
    """the inputs of test_width_classes_gpu.py::test_lll_ex_against_exact_arithmetic.  Short-wide: b reaches every
    chunk of the lanes, u (16 .. 24 columns) the first alone — the lanes of the other chunks must leave u alone.
    Tall (180 and 200 rows): rows and columns of u in chunks 3 and 4.  The unique u comes from exact elimination on the
    short-wide inputs and from the verified proposal of hlll_transform_cases on the square tall ones."""
    bs = W.short_wide_batch(*case[1:]) if case[0] == "short" else W.tall_batch(case[1])
    k = len(bs)
    t = time.time()
    st, info, out, u, _, ms = X.tracked_and_twin(ctx, bs, lambda g: g.lll_ex(prec))
    t_run = time.time() - t
    assert list(st) == [1] * (2 * k), (st, info)
    for L, b in enumerate(bs):
        assert int(info[L][1]) > 0
        T.check_transform(u[L], b, out[L])
    C.note(lambda: ("lll_ex(%d) with u %s NQ %d: swaps %s, kernel %.1f ms, both runs %.1f s, test %.1f s"
                    % (prec, _wide_id(case), W.nq_of(*bs[0].shape), [int(i[1]) for i in info[:k]], ms, t_run,
                       time.time() - t),))


# ---- 6. the ladder ------------------------------------------------------------------------------------------------------------------
def test_ladder_keeps_u_in_step_across_the_stages(ctx, monkeypatch):
    """FPHIP_LLL_LADDER_TEST=2: the odd lattices go on in double-double and every fourth in quad-double, each stage
    from the b AND the u the stage before left on the device.  Four copies of lll_q40 and four unimodular variants of
    it.  The lattices that stay at 53 bits are skipped by both later launches, which write every row of the batch in
    position order: their u must be the u of lll() alone (u2 := u before each launch)."""
    f = X.lll_fixture("lll_q40")
    d = f["d"]
    bs = [f["b_in"]] * 4 + [W._matmul_exact(T.seeded_unimodular(d, s), f["b_in"]) for s in range(4)]
    run = lambda g: g.lll_ladder(f["kmin"], f["kstart"], f["kend"], f["delta"], f["eta"])  # noqa: E731
    single = X.gso(ctx, bs)   # the first stage alone, with u: before the test level is set
    single.enable_transform()
    st1, _ = single.lll(f["kmin"], f["kstart"], f["kend"], f["delta"], f["eta"])
    u1, out1 = single.get_transform(), single.get_basis(0, 8)
    single.close()
    assert list(st1) == [1] * 8
    monkeypatch.setenv("FPHIP_LLL_LADDER_TEST", "2")
    twin = X.gso(ctx, bs)
    want = run(twin)
    want_out = twin.get_basis(0, 8)
    twin.close()
    g = X.gso(ctx, bs)
    g.enable_transform()
    st, info, stage = run(g)
    out, u = g.get_basis(0, 8), g.get_transform()
    g.close()
    assert list(st) == [1] * 8
    assert list(stage) == [53, 106, 53, 212, 53, 106, 53, 212]
    for a, b in zip((st, info, stage), want):
        assert np.array_equal(a, b)
    assert np.array_equal(out, want_out)
    for L in range(8):
        X.relation(u[L], bs[L], out[L])
    for L in (0, 2, 4, 6):
        assert np.array_equal(u[L], u1[L]) and np.array_equal(out[L], out1[L]), L
    for L in range(4):
        assert np.array_equal(out[L], f["b_out"])
        T.check_transform(u[L], f["b_in"], f["b_out"])


def test_ladder_on_a_wide_shape(ctx, monkeypatch):
    """test level 1 on 20 x 193 (four columns per lane), the case test_width_classes_gpu.py runs untracked: the odd
    lattices go on in double-double, every lattice ends on the oracle's basis, u follows.  (A tracked u at this width
    has no quad-double stage; double-double succeeds on these bases, as the untracked test shows first.)"""
    bs = W.short_wide_batch(20, 193)
    monkeypatch.setenv("FPHIP_LLL_LADDER_TEST", "1")
    g = X.gso(ctx, bs)
    g.enable_transform()
    st, info, stage = g.lll_ladder()
    out, u = g.get_basis(0, 5), g.get_transform()
    g.close()
    assert list(st) == [1] * 5 and list(stage) == [53, 106, 53, 106, 53]
    for L, b in enumerate(bs):
        assert np.array_equal(out[L], W.oracle_lll(b)[2]), L
        T.check_transform(u[L], b, out[L])


# ---- 7. a multiplier beyond 63 bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [53, 106, 212])
def test_multiplier_overflow_leaves_b_and_u_in_step(ctx, prec):
    """row 2 = (2^63 - 1, 5, 1) against the unit vectors: the multiplier against row 1 fits, the one against row 0 does
    not — the kernel has updated its copies of both rows by then and must drop BOTH.  Whatever the status, u describes
    the b on the device."""
    b = np.array([[1, 0, 0], [0, 1, 0], [2 ** 63 - 1, 5, 1]], dtype=np.int64)
    st, info, out, u, _, _ = X.tracked_and_twin(ctx, [b], lambda g: g.lll_ex(prec))
    C.note(lambda: ("multiplier overflow at %d bits: status %s, info %s" % (prec, list(st), info.tolist()),))
    assert np.array_equal(u[0].astype(object).dot(b.astype(object)), out[0].astype(object))
    assert T.is_unimodular(u[0])


# ---- 8. the quad-double limit -------------------------------------------------------------------------------------------------------------
def test_quad_double_with_u_refuses_more_than_64_columns(ctx):
    """lll_ex(212) with a tracked u and max(d, n) > 64 is refused before anything is launched, says why, leaves b and u
    alone, and the object goes on working.  (The same object WITHOUT u is not launched at 212 bits here.)"""
    import fplll_amd
    bs = W.short_wide_batch(16, 128, 2)
    u0 = np.stack([T.seeded_unimodular(16, s) for s in (1, 2)])
    g = X.gso(ctx, bs)
    g.enable_transform(u0)
    with pytest.raises(fplll_amd.HipError, match=r"quad-double.*max\(d, n\) <= 64"):
        g.lll_ex(212)
    assert np.array_equal(g.get_basis(0, 2), np.stack(bs)) and np.array_equal(g.get_transform(), u0)
    st, _ = g.lll_ex(106)
    assert list(st) == [1, 1]
    out, u = g.get_basis(0, 2), g.get_transform()
    g.close()
    from fplll_amd.gso import inverse_transpose
    for L in range(2):   # u = T u0 with T b = b_out
        Tm = W._matmul_exact(u[L].astype(object), inverse_transpose(u0[L]).T)
        X.relation(Tm, bs[L], out[L])


# ---- 9. housekeeping ----------------------------------------------------------------------------------------------------------------------
def test_housekeeping(ctx):
    import fplll_amd
    f = X.lll_fixture("lll_q40")
    d, b_in = f["d"], f["b_in"]
    eye = np.eye(d, dtype=np.int64)
    # without enable_transform: what lll_ex returns today, and no transformation to read
    g = X.gso(ctx, [b_in] * 2)
    st, info = g.lll_ex(106, f["kmin"], f["kstart"], f["kend"], f["delta"], f["eta"])
    assert list(st) == [1, 1] and np.array_equal(g.get_basis(0, 1)[0], f["b_out"]) and int(info[0][1]) == f["n_swaps"]
    with pytest.raises(fplll_amd.HipError, match="enable_transform"):
        g.get_transform()
    # lll_ex twice: the first 20 rows, then all of them — u accumulates
    g.set_basis(np.stack([b_in] * 2))
    g.enable_transform()
    st, _ = g.lll_ex(106, 0, 0, 20, f["delta"], f["eta"])
    assert list(st) == [1, 1]
    u_a, out_a = g.get_transform(), g.get_basis(0, 2)
    X.relation(u_a[0], b_in, out_a[0])
    assert np.array_equal(u_a[0][20:], eye[20:]) and not np.array_equal(u_a[0], eye)
    st, _ = g.lll_ex(53, 0, 0, -1, f["delta"], f["eta"])
    assert list(st) == [1, 1]
    u_b, out_b = g.get_transform(), g.get_basis(0, 2)
    assert not np.array_equal(u_b[0], u_a[0])
    T.check_transform(u_b[0], b_in, out_b[0])
    assert np.array_equal(u_b[0], u_b[1])
    # set_basis keeps u; enabling again resets it
    g.set_basis(b_in, first=1)
    assert np.array_equal(g.get_transform(), u_b)
    g.set_basis(b_in, first=0)
    g.enable_transform()
    assert np.array_equal(g.get_transform(), np.stack([eye] * 2))
    # lll() then lll_ex(106): across the two kernels
    st, _ = g.lll(0, 0, 20, f["delta"], f["eta"])
    assert list(st) == [1, 1]
    u_c = g.get_transform()
    X.relation(u_c[0], b_in, g.get_basis(0, 1)[0])
    st, _ = g.lll_ex(106, 0, 0, -1, f["delta"], f["eta"])
    assert list(st) == [1, 1]
    u_d, out_d = g.get_transform(), g.get_basis(0, 2)
    assert not np.array_equal(u_d[0], u_c[0])
    T.check_transform(u_d[0], b_in, out_d[0])
    # the inverse transpose, derived from the u the device tracks
    uinv_t = g.get_inverse_transform_t()
    for L in range(2):
        prod = W._matmul_exact(uinv_t[L].T.astype(object), u_d[L].astype(object))
        assert np.array_equal(prod, np.eye(d, dtype=object)), L
    # the entry points that do not update u still refuse it
    with pytest.raises(fplll_amd.HipError, match="does not update it"):
        g.size_reduction()
    g.close()


# ---- 10. the public entry -----------------------------------------------------------------------------------------------------------------
def test_lll_reduction(ctx):
    """gso.lll_reduction on an UNREDUCED 40-dimensional q-ary basis: u b = b_out for every method the device covers,
    method="fast" returns the basis of MatGSOBatch.lll(), the wrapper stays at 53 bits, with_u=False returns no u."""
    from fplll_amd import gso
    d = 40
    b = X.qary(np.random.default_rng(77), d, d // 2, 4099)
    assert X.full_row_rank(b)
    g = X.gso(ctx, [b])
    st, _ = g.lll()
    assert list(st) == [1]
    b_lll = g.get_basis(0, 1)[0]
    g.close()
    assert not np.array_equal(b_lll, b)
    for method, float_type, stage_want in (("fast", "double", 53), ("fast", "dd", 106), ("fast", "qd", 212),
                                           ("wrapper", "double", 53)):
        b_out, u, st, stage = gso.lll_reduction(ctx, b, method=method, float_type=float_type)
        assert st == 1 and stage == stage_want and b_out.shape == (d, d) and u.shape == (d, d)
        T.check_transform(u, b, b_out)
        if (method, float_type) in (("fast", "double"), ("wrapper", "double")):
            assert np.array_equal(b_out, b_lll)
    b_out, u, st, stage = gso.lll_reduction(ctx, np.stack([b, b_lll]), with_u=False, method="fast")
    assert u is None and list(st) == [1, 1] and list(stage) == [53, 53] and b_out.shape == (2, d, d)
    assert np.array_equal(b_out[0], b_lll) and np.array_equal(b_out[1], b_lll)
    b_out, u, st, stage = gso.lll_reduction(ctx, np.stack([b, b_lll]))
    assert u.shape == (2, d, d) and list(stage) == [53, 53]
    for L, b_in in enumerate((b, b_lll)):
        T.check_transform(u[L], b_in, b_out[L])
