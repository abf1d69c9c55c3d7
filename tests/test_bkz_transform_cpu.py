"""The transformation matrix u through the device BKZ entry points (FPHIP_BKZ_TRANSFORM), CPU side: the interface
(header, ctypes mirror, ABI version, Python signatures, build list) and the MODEL of what the kernels do to u — a
pure-numpy replay of the reference's three insertion procedures (svp_postprocessing, bkz.cpp:126-203; its generic
gcd tree, :205-272; both with dual = false and dual = true) applied to an identity u.  The kernels
(bkz_kernel.hip / bkzs_kernel.hip compiled with FPHIP_BKZ_U) apply the same operations to the same rows of u; the
GPU side (test_bkz_transform_gpu.py) checks them by u b_in = b_out."""
import inspect
import os
import re

import numpy as np
import pytest

import conftest as C


# ---- the model ---------------------------------------------------------------------------------------------------------
def move_row(u, old, new):
    """MatGSO::move_row(old, new), gso.cpp:289-366: the row at `old` goes to `new`, the rows in between shift by one"""
    rows = list(range(u.shape[0]))
    rows.insert(new, rows.pop(old))
    return u[rows]


def row_addmul(u, i, j, x):
    """row_addmul(i, j, x): u[i] += x u[j]"""
    u[i] = u[i] + int(x) * u[j]


def postprocess(u, kappa, x, dual=False):
    """svp_postprocessing(kappa, len(x), x, dual) on u (an object array, changed in place and returned; move_row
    returns a new array).  Returns (u, kind): 'rotate', 'unit' or 'generic'."""
    x = [int(v) for v in x]
    bs = len(x)
    nz = sum(1 for v in x if v != 0)
    ones = [i for i in range(bs) if abs(x[i]) == 1]
    iv = ones[-1] if ones else -1            # the LAST +-1 (the reference scans from the top, bkz.cpp:131-141)
    pos = kappa + bs - 1 if dual else kappa
    if nz == 1:
        return move_row(u, kappa + iv, pos), "rotate"
    if iv != -1:
        dd = -x[iv] if dual else x[iv]
        for i in range(bs):
            if x[i] != 0 and i != iv:
                if dual:
                    row_addmul(u, kappa + i, kappa + iv, dd * x[i])
                else:
                    row_addmul(u, kappa + iv, kappa + i, dd * x[i])
        return move_row(u, kappa + iv, pos), "unit"
    # svp_postprocessing_generic: gcd tree on |x|
    for i in range(bs):
        if x[i] < 0:
            x[i] = -x[i]
            u[kappa + i] = -u[kappa + i]     # negate_row_of_b
    off = 1
    while off < bs:
        k = bs - 1
        while k - off >= 0:
            if x[k] != 0 or x[k - off] != 0:
                if x[k] < x[k - off]:
                    x[k], x[k - off] = x[k - off], x[k]
                    u[[kappa + k - off, kappa + k]] = u[[kappa + k, kappa + k - off]]
                while x[k - off] != 0:
                    while x[k - off] <= x[k]:
                        x[k] -= x[k - off]
                        if dual:
                            row_addmul(u, kappa + k, kappa + k - off, -1)      # row_sub(k, k - off)
                        else:
                            row_addmul(u, kappa + k - off, kappa + k, 1)       # row_add(k - off, k)
                    x[k], x[k - off] = x[k - off], x[k]
                    u[[kappa + k - off, kappa + k]] = u[[kappa + k, kappa + k - off]]
            k -= 2 * off
        off *= 2
    assert x == [0] * (bs - 1) + [1], "the coefficients of a shortest vector are coprime"
    if not dual:
        u = move_row(u, kappa + bs - 1, kappa)
    return u, "generic"


def bareiss_det(m):
    import wide_cases as W
    return W.bareiss_det(m)


D, KAPPA = 9, 2   # the block sits inside a larger basis: rows outside [KAPPA, KAPPA + bs) must not move


def _embedded(x):
    full = [0] * D
    full[KAPPA:KAPPA + len(x)] = [int(v) for v in x]
    return np.array(full, dtype=object)


PRIMAL = [((0, 0, 1, 0), "rotate"), ((-1, 0, 0, 0, 0), "rotate"), ((0, -1), "rotate"),
          ((2, -1, 0, 3), "unit"), ((1, 5, -1, 0, 2), "unit"), ((3, 0, 1), "unit"), ((-1, -1), "unit"),
          ((2, 3, 0, 5), "generic"), ((-2, 3), "generic"), ((6, -10, 15), "generic"), ((0, 4, -7, 0, 2, 9), "generic"),
          ((5, 0, 0, 0, 0, 0, 3), "generic")]


@pytest.mark.parametrize("x,kind", PRIMAL, ids=lambda v: str(v).replace(" ", ""))
def test_primal_insertion_replay_puts_the_vector_at_kappa(x, kind):
    """u stays unimodular, rows outside the block stay, and row kappa of u is the coefficient vector of the
    inserted vector (up to the sign of x_iv in the +-1 cases: b'_kappa = x_iv sum x_i b_i)."""
    u, got = postprocess(np.array(np.eye(D, dtype=np.int64), dtype=object), KAPPA, x)
    assert got == kind
    assert abs(bareiss_det(u)) == 1
    want = _embedded(x)
    assert np.array_equal(u[KAPPA], want) or (kind != "generic" and np.array_equal(u[KAPPA], -want))
    bs = len(x)
    for r in list(range(KAPPA)) + list(range(KAPPA + bs, D)):
        assert np.array_equal(u[r], np.eye(D, dtype=np.int64)[r])
    # the other rows of the block still span the block with the new row kappa
    blk = u[KAPPA:KAPPA + bs, KAPPA:KAPPA + bs]
    assert abs(bareiss_det(blk)) == 1


DUAL = [((0, 1, 0), "rotate"), ((2, 1, -3), "unit"), ((-1, 0, 4, 1, 0), "unit"),
        ((2, 3, 0, 5), "generic"), ((-3, 2), "generic"), ((6, 10, -15, 0), "generic")]


@pytest.mark.parametrize("x,kind", DUAL, ids=lambda v: str(v).replace(" ", ""))
def test_dual_insertion_replay_puts_the_dual_vector_last(x, kind):
    """dual = true: with b' = U b the dual basis is d' = U^-T d, and the LAST dual vector of the block must be
    sum x_i d_i (up to the sign of x_iv): row (U^-T)[last] = +-x, which is U x = +-e_last — no inverse needed."""
    u, got = postprocess(np.array(np.eye(D, dtype=np.int64), dtype=object), KAPPA, x, dual=True)
    assert got == kind
    assert abs(bareiss_det(u)) == 1
    last = KAPPA + len(x) - 1
    e = np.array([1 if i == last else 0 for i in range(D)], dtype=object)
    ux = u.dot(_embedded(x))
    assert np.array_equal(ux, e) or (kind != "generic" and np.array_equal(ux, -e))
    for r in list(range(KAPPA)) + list(range(last + 1, D)):
        assert np.array_equal(u[r], np.eye(D, dtype=np.int64)[r])


def test_replay_acts_on_a_basis_like_on_u():
    """the same operations on b and on u = identity: u b_in = b_out (what the GPU tests assert of the kernels)"""
    rng = np.random.default_rng(11)
    b_in = np.array(rng.integers(-50, 51, size=(D, D)), dtype=object)
    for x, dual in [((2, 3, 0, 5), False), ((2, -1, 0, 3), False), ((2, 3, 0, 5), True), ((2, 1, -3), True)]:
        u, _ = postprocess(np.array(np.eye(D, dtype=np.int64), dtype=object), KAPPA, x, dual)
        b, _ = postprocess(b_in.copy(), KAPPA, x, dual)
        assert np.array_equal(u.dot(b_in), b)
        if not dual:
            assert np.array_equal(b[KAPPA], _embedded(x).dot(b_in)) or np.array_equal(b[KAPPA], -_embedded(x).dot(b_in))


# ---- the interface -----------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(C.ROOT, "include", "fplll_hip.h")) as f:
        return f.read()


def test_header_defines_the_flag_and_the_mirror_agrees():
    from fplll_amd import _lib
    m = re.search(r"^#define\s+FPHIP_BKZ_TRANSFORM\s+(0x[0-9a-fA-F]+)", _header(), re.M)
    assert m and int(m.group(1), 16) == 0x4000 == _lib.FPHIP_BKZ_TRANSFORM
    # no other FPHIP_BKZ_* flag shares the bit
    others = {n: int(v, 16) for n, v in re.findall(r"^#define\s+(FPHIP_BKZ_\w+)\s+(0x[0-9a-fA-F]+)", _header(), re.M)
              if n != "FPHIP_BKZ_TRANSFORM"}
    assert others and all(v & 0x4000 == 0 for v in others.values())
    assert "fphip_gso_bkz_insert_stats" in _header()


def test_abi_version_and_the_debug_getter_resolve():
    from fplll_amd import _lib
    lib = _lib.load()
    assert lib.fphip_abi_version() >= 4
    assert lib.fphip_gso_bkz_insert_stats is not None


def test_python_entry_points_take_transform():
    from fplll_amd import gso
    for fn in (gso.MatGSOBatch.bkz, gso.MatGSOBatch.bkz_strategies):
        p = inspect.signature(fn).parameters
        assert "transform" in p and p["transform"].default is False
    assert callable(gso.MatGSOBatch.bkz_insert_stats)
    p = inspect.signature(gso.bkz_reduction).parameters
    assert list(p)[:4] == ["ctx", "b", "block_size", "strategies"] and p["with_u"].default is True


def test_the_u_kernels_are_built_with_the_flags_of_their_twins():
    from fplll_amd import build
    for twin, mine in (("bkz_kernel.hip", "bkz_kernel_u.hip"), ("bkzs_kernel.hip", "bkzs_kernel_u.hip")):
        assert mine in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC, mine))
        assert build.PER_FILE_FLAGS[mine] == build.PER_FILE_FLAGS[twin]
        assert twin in build.EXTRA_DEPS[mine]
