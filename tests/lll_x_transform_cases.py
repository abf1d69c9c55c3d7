"""What tests/test_lll_x_transform_gpu.py runs on every input: the tracked object next to its untracked twin.

A launch holds every basis twice — lattices 0 .. k-1 with u = identity, lattices k .. 2k-1 with an uploaded unimodular
u0 (hlll_transform_cases.seeded_unimodular) — and a second object without u runs the same call on the same 2k bases.
Tracking must change nothing of the run (status, info, basis: those of the twin), and the kernel applies ONE sequence
of row operations T to whatever u it finds: u[k + L] = u[L] u0[L] in exact integers.  What u[L] itself must be is the
business of each test (hlll_transform_cases.check_transform against the basis the device returns)."""
import functools
import os

import numpy as np
import pytest

import conftest as C
import hlll_transform_cases as T
import wide_cases as W


@functools.lru_cache(maxsize=None)
def lll_fixture(name):
    return C.load_lll_fixture(os.path.join(C.GOLDEN, name + ".json"))


def full_row_rank(b):
    """a PROOF that the rows of b are independent: a d x d minor with a non-zero determinant modulo a prime (the
    square basis itself, or b without one of its columns when it has d + 1).  False proves nothing."""
    b = np.asarray(b, dtype=np.int64)
    d, n = b.shape
    if d == n:
        return T.nonsingular_mod_p(b)
    assert n == d + 1
    return any(T.nonsingular_mod_p(np.delete(b, j, axis=1)) for j in range(n - 1, -1, -1))


def gso(ctx, bs):
    from fplll_amd.gso import MatGSOBatch
    g = MatGSOBatch(ctx, len(bs), *bs[0].shape)
    g.set_basis(np.stack(bs))
    return g


def tracked_and_twin(ctx, bs, run, seed=1):
    """run(g) -> (status, info, ...) on the tracked object (module docstring) and on its twin; asserts that tracking
    changes nothing and that the uploaded u0 is multiplied from the left.  Returns (status, info, b_out[2k], u[2k], u0[k])
    of the tracked run."""
    k, d = len(bs), bs[0].shape[0]
    eye = np.eye(d, dtype=np.int64)
    u0 = [T.seeded_unimodular(d, seed + L) for L in range(k)]
    assert all(not np.array_equal(m, eye) for m in u0)
    both = list(bs) + list(bs)
    twin = gso(ctx, both)
    want = run(twin)
    want_out = twin.get_basis(0, 2 * k)
    import fplll_amd
    with pytest.raises(fplll_amd.HipError, match="enable_transform"):   # an object that never enabled it has none
        twin.get_transform()
    twin.close()
    g = gso(ctx, both)
    u_in = np.stack([eye] * k + u0)
    g.enable_transform(u_in)
    assert np.array_equal(g.get_transform(), u_in)
    got = run(g)
    out, u = g.get_basis(0, 2 * k), g.get_transform()
    ms = g.last_kernel_ms
    g.close()
    for a, b in zip(got, want):   # status, info (and stage)
        assert np.array_equal(a, b), (a, b)
    assert np.array_equal(out, want_out)
    assert u.shape == (2 * k, d, d) and u.dtype == np.int64
    for L in range(k):
        assert W._matmul_equals(u[L], u0[L], u[k + L]), L
    return got[0], got[1], out, u, u0, ms


def relation(u, b_in, b_out):
    """u b_in = b_out in exact integers and |det u| = 1: what holds whether or not u is determined by the bases"""
    T.check_transform(u, b_in, b_out, unique=False)


def qary(rng, d, k, q):
    b = np.zeros((d, d), dtype=np.int64)
    b[:k, :k] = np.eye(k, dtype=np.int64)
    b[:k, k:] = rng.integers(0, q, size=(k, d - k))
    b[k:, k:] = q * np.eye(d - k, dtype=np.int64)
    return b
