"""The transformation matrix u on the Householder objects (MatHouseholderBatch.enable_transform /
fphip_hh_enable_transform): after every entry point that changes b, u_out = T u_in where b_out = T b_in.

The reference for u is the UNIQUE integer U with U b_in = b_out for the reference's b_out (fixtures, C oracle):
tests/hlll_transform_cases.py computes it, tests/test_hlll_transform_cpu.py shows it sound on these very inputs.  Where
the device's basis need not be the oracle's (the tree-sum kernels), u is checked against the device's own b_out: the
product identity in exact integers and |det u| = 1."""
import os

import numpy as np
import pytest

import conftest as C
import hlll_transform_cases as T
import wide_cases as W

pytestmark = pytest.mark.gpu


def _hh(ctx, bs, row_expo=True):
    from fplll_amd.householder import MatHouseholderBatch
    h = MatHouseholderBatch(ctx, len(bs), *bs[0].shape, row_expo=row_expo)
    h.set_basis(np.stack(bs))
    return h


# ---- 1. the reference's fixtures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.HLLL_FIXTURES)
def test_fixture_transform_is_the_references(ctx, name):
    """tracking changes nothing of the run (status, basis, swaps and iterations are the fixture's and the oracle's), and
    u is the one matrix that takes b_in to b_out"""
    f = T.hlll_fixture(name)
    h = _hh(ctx, [f["b_in"]] * 3)
    h.enable_transform()
    st, info = h.hlll(f["delta"], f["eta"], f["theta"], f["c"])
    assert list(st) == [f["status"]] * 3
    out, u = h.get_basis(0, 3), h.get_transform()
    ost, ob, oinfo = C.oracle_hlll(f["b_in"], f["delta"], f["eta"], f["theta"], f["c"])
    assert u.shape == (3, f["d"], f["d"]) and u.dtype == np.int64
    for L in range(3):
        assert np.array_equal(out[L], f["b_out"]) and np.array_equal(out[L], ob)
        assert list(info[L]) == list(oinfo)
        T.check_transform(u[L], f["b_in"], f["b_out"])
    assert h.last_kernel_ms > 0
    h.close()


# ---- 2. a u that does not start at the identity ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hlll_q40", "hlll_u24"])
def test_uploaded_transform_is_multiplied_from_the_left(ctx, name):
    """get_transform() = T u0 for three different unimodular u0, T being what the identity run of the same lattice
    returns: the unique transformation of the fixture (test_fixture_transform_is_the_references)"""
    f = T.hlll_fixture(name)
    d = f["d"]
    u0 = np.stack([T.seeded_unimodular(d, s) for s in (1, 2, 3)])
    assert all(not np.array_equal(m, np.eye(d, dtype=np.int64)) for m in u0)
    Tm = T.unique_transform(f["b_in"], f["b_out"])
    h = _hh(ctx, [f["b_in"]] * 3)
    h.enable_transform(u0)
    assert np.array_equal(h.get_transform(), u0)
    st, _ = h.hlll(f["delta"], f["eta"], f["theta"], f["c"])
    assert list(st) == [1] * 3
    u = h.get_transform()
    for L in range(3):
        assert W._matmul_equals(Tm, u0[L], u[L]), L
    h.close()


# ---- 3. different lattices in one launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n_extra", T.HETEROGENEOUS)
def test_heterogeneous_batch(ctx, d, n_extra):
    """six different lattices: waves 1 .. 3 of the first workgroup and a second workgroup — the batch and row strides
    of u ([batch][d][ldu], ldu padded) with d that are no multiple of the padding, and one shape with n > d"""
    bs = T.heterogeneous_batch(d, n_extra)
    assert len(bs) >= 6
    h = _hh(ctx, bs)
    h.enable_transform()
    st, info = h.hlll()
    out, u = h.get_basis(0, len(bs)), h.get_transform()
    for L, b in enumerate(bs):
        ost, oinfo, ob = W.oracle_hlll(b)
        assert st[L] == ost == 1, (L, st)
        assert tuple(int(x) for x in info[L]) == oinfo, L
        assert np.array_equal(out[L], ob), L
        T.check_transform(u[L], b, ob)
    h.close()


# ---- 4. every columns-per-lane instantiation -----------------------------------------------------------------------------
WIDE = [("short", d, n) for d, n in W.SHORT_WIDE] + [("tall", 3), ("tall", 4)]


def _wide_id(case):
    return "%dx%d" % case[1:] if case[0] == "short" else "tall%d" % W.tall_base(case[1]).shape[0]


def _wide_inputs(case):
    return W.short_wide_batch(*case[1:]) if case[0] == "short" else W.tall_batch(case[1])


@pytest.mark.parametrize("case", WIDE, ids=_wide_id)
def test_every_nq(ctx, case):
    """hlll_u_kernel<2, 3, 4> on the inputs of test_width_classes_gpu.py::test_hlll_matches_oracle; on the tall batches
    the rows and the columns of u reach every chunk and four exchanges lie in the last one"""
    bs = _wide_inputs(case)
    h = _hh(ctx, bs)
    h.enable_transform()
    st, info = h.hlll()
    out, u = h.get_basis(0, len(bs)), h.get_transform()
    for L, b in enumerate(bs):
        ost, oinfo, ob = W.oracle_hlll(b)
        assert st[L] == ost == 1, (L, st)
        assert tuple(int(x) for x in info[L]) == oinfo, L
        assert np.array_equal(out[L], ob), L
        T.check_transform(u[L], b, ob)
    C.note(lambda: ("hlll with u %s NQ %d: swaps %s, kernel %.1f ms"
                    % (_wide_id(case), (bs[0].shape[1] + 63) // 64, [int(i[0]) for i in info], h.last_kernel_ms),))
    h.close()


# ---- 5. the tree-sum kernels ---------------------------------------------------------------------------------------------
def _precision_inputs(case):
    if case[0] == "short":
        return W.short_wide_batch(*case[1:])
    f = T.hlll_fixture(case[1])
    return [f["b_in"]] * 2


PRECISION = ([(c, p) for c in [("short", d, n) for d, n in W.SHORT_WIDE] + [("fix", "hlll_q40"), ("fix", "hlll_r30")]
              for p in (53, 106)] + [(("fix", "hlll_q40"), 212), (("fix", "hlll_r30"), 212)])


@pytest.mark.parametrize("case,precision", PRECISION,
                         ids=["%s-%d" % (c[1] if c[0] == "fix" else "%dx%d" % c[1:], p) for c, p in PRECISION])
def test_selectable_precision(ctx, case, precision):
    """hlll(precision = 53 / 106 / 212): hlll_x_u_kernel.  The basis need not be the oracle's there, so u is held
    against the basis the device returns."""
    bs = _precision_inputs(case)
    h = _hh(ctx, bs)
    h.enable_transform()
    st, info = h.hlll(precision=precision)
    assert list(st) == [1] * len(bs), st
    out, u = h.get_basis(0, len(bs)), h.get_transform()
    for L, b in enumerate(bs):
        assert int(info[L][0]) > 0   # (the run did exchange rows)
        T.check_transform(u[L], b, out[L], unique=False)
    h.close()


# ---- 6. the precision ladder -----------------------------------------------------------------------------------------------
def test_ladder_keeps_u_in_step_across_the_stages(ctx, monkeypatch):
    """FPHIP_HLLL_LADDER_TEST=2: the odd lattices go on in double-double and every fourth in quad-double, each stage
    from the b AND the u the stage before left on the device.  Four copies of hlll_q40 and four unimodular variants
    of it, so that the later stages see different bases."""
    f = T.hlll_fixture("hlll_q40")
    bs = [f["b_in"]] * 4 + [W._matmul_exact(T.seeded_unimodular(f["d"], s), f["b_in"]) for s in range(4)]
    monkeypatch.setenv("FPHIP_HLLL_LADDER_TEST", "2")
    h = _hh(ctx, bs)
    h.enable_transform()
    st, info, stage = h.hlll_ladder(f["delta"], f["eta"], f["theta"], f["c"])
    assert list(st) == [1] * 8
    assert list(stage) == [53, 106, 53, 212, 53, 106, 53, 212]
    out, u = h.get_basis(0, 8), h.get_transform()
    for L in range(8):
        T.check_transform(u[L], bs[L], out[L], unique=False)
    for L in range(4):
        assert np.array_equal(out[L], f["b_out"])
        T.check_transform(u[L], f["b_in"], f["b_out"])
    h.close()


# ---- 7. the stand-alone size reduction -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", C.hhsr_fixtures(), ids=lambda p: os.path.basename(p)[:-5])
def test_size_reduce(ctx, path):
    f = C.load_hhsr_fixture(path)
    k, d = f["kappa"], f["d"]
    b_in, b_out = T.hhsr_pair(f)
    h = _hh(ctx, [b_in] * 5, row_expo=bool(f["row_expo_on"]))
    h.enable_transform()
    assert list(h.update_R()) == [1] * 5
    assert np.array_equal(h.get_transform(), np.stack([np.eye(d, dtype=np.int64)] * 5))   # update_R leaves b alone
    red, st = h.size_reduce(k, f["end"], f["start"])
    assert list(red) == [f["reduced"]] * 5 and list(st) == [1] * 5
    b, u = h.get_basis(0, 5), h.get_transform()
    others = np.arange(d) != k
    for L in range(5):
        assert np.array_equal(b[L], b_out)
        assert np.array_equal(u[L][others], np.eye(d, dtype=np.int64)[others])
        assert u[L][k, k] == 1 and not np.any(u[L][k, k + 1:])
        assert np.any(u[L][k, :k]) == bool(f["reduced"])
        T.check_transform(u[L], b_in, b_out)
    h.close()


# ---- 8. housekeeping -------------------------------------------------------------------------------------------------------
def test_housekeeping(ctx):
    import fplll_amd
    f = T.hlll_fixture("hlll_u24")
    d = f["d"]
    eye = np.eye(d, dtype=np.int64)
    h = _hh(ctx, [f["b_in"]] * 3)
    with pytest.raises(fplll_amd.HipError, match="enable_transform"):
        h.get_transform()
    # an object that never enables it: the plain path, the fixture's result
    st, info = h.hlll(f["delta"], f["eta"], f["theta"], f["c"])
    assert list(st) == [1] * 3 and np.array_equal(h.get_basis(0, 1)[0], f["b_out"])
    assert h.last_kernel_ms > 0
    with pytest.raises(fplll_amd.HipError):
        h.get_transform()
    # lattice 0 reduced with u, the others waiting: set_basis keeps u, broadcast_basis copies it, enabling again resets
    h.set_basis(np.stack([f["b_in"], f["b_out"], f["b_out"]]))
    h.enable_transform()
    st, _ = h.hlll(f["delta"], f["eta"], f["theta"], f["c"])
    assert list(st) == [1] * 3
    u = h.get_transform()
    T.check_transform(u[0], f["b_in"], f["b_out"])
    assert not np.array_equal(u[0], eye)
    h.set_basis(f["b_in"], first=1)
    assert np.array_equal(h.get_transform(), u)
    h.broadcast_basis(0)
    assert np.array_equal(h.get_transform(), np.stack([u[0]] * 3))
    assert all(np.array_equal(b, f["b_out"]) for b in h.get_basis(0, 3))
    assert np.array_equal(h.get_transform(1, 2), np.stack([u[0]] * 2))
    h.enable_transform()
    assert np.array_equal(h.get_transform(), np.stack([eye] * 3))
    h.close()


def test_more_rows_than_columns_is_declined(ctx):
    from fplll_amd.householder import MatHouseholderBatch
    try:
        h = MatHouseholderBatch(ctx, 1, 6, 4, row_expo=True)
    except Exception:
        return   # (such a shape is not accepted at all)
    with pytest.raises(NotImplementedError, match="d = 6"):
        h.enable_transform()
    h.close()


# ---- 9. the inverse transpose ----------------------------------------------------------------------------------------------
def test_inverse_transform_t(ctx):
    f = T.hlll_fixture("hlll_q40")
    d = f["d"]
    h = _hh(ctx, [f["b_in"]] * 2)
    h.enable_transform()
    st, _ = h.hlll(f["delta"], f["eta"], f["theta"], f["c"])
    assert list(st) == [1, 1]
    u, uinv_t = h.get_transform(), h.get_inverse_transform_t()
    assert uinv_t.shape == (2, d, d)
    for L in range(2):
        prod = W._matmul_exact(uinv_t[L].T.astype(object), u[L].astype(object))
        assert np.array_equal(prod, np.eye(d, dtype=object)), L
    assert h.get_inverse_transform_t(1, 1).shape == (1, d, d)
    h.close()
