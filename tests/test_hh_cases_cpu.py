"""The inputs and checkers of tests/hh_cases.py are what they claim to be — on the CPU, with the C oracle
(oracle/hh_oracle.c: the reference's update_R in its own order) and exact arithmetic: every shape reaches the
instantiation, panel count and ragged edge its table claims; the oracle's R is within 2^-44 of the true factor on every
input (a condition on the INPUTS: it keeps the GPU gate, 2^4 above the exact mode's error, below the project's 53-bit
gate for R, 2^-40); the `tri` and `zero_row` families have the exact answers the GPU test asserts; and the checker
rejects doctored results."""
import numpy as np
import pytest

import conftest as C
import ftx_cases as F
import hh_cases as H
import wide_cases as W

CAP = 2.0 ** -44

# (d, n): NQ, panels, rows of the last panel, columns of the last tile, columns of the last 64-chunk, LDS stride
TABLE = {(1, 1): (1, 1, 1, 1, 1, 33), (1, 5): (1, 1, 1, 5, 5, 33), (15, 15): (1, 1, 15, 15, 15, 33),
         (16, 16): (1, 1, 16, 16, 16, 33), (17, 17): (1, 2, 1, 1, 17, 33), (33, 40): (1, 3, 1, 8, 40, 65),
         (64, 64): (1, 4, 16, 16, 64, 65),
         (17, 65): (2, 2, 1, 1, 1, 97), (48, 128): (2, 3, 16, 16, 64, 129), (65, 65): (2, 5, 1, 1, 1, 97),
         (100, 128): (2, 7, 4, 16, 64, 129),
         (17, 129): (3, 2, 1, 1, 1, 161), (33, 192): (3, 3, 1, 16, 64, 193), (129, 129): (3, 9, 1, 1, 1, 161),
         (17, 193): (4, 2, 1, 1, 1, 225), (49, 208): (4, 4, 1, 16, 16, 225), (32, 256): (4, 2, 16, 16, 64, 257)}


def _sid(shape):
    return "%dx%d" % shape


def test_every_shape_reaches_what_its_table_claims():
    """the launcher's formulas (fphip_hh_update_R_blocked: nq, nblk, ldx, lds, bpc, grid), restated in hh_cases"""
    assert set(TABLE) == set(H.ALL_SHAPES)
    for nq, shapes in H.SHAPES.items():
        for d, n in shapes:
            assert d <= n and H.nq_of(n) == nq
            got = (H.nq_of(n), H.panels(d), d - 16 * (H.panels(d) - 1), H.last_tile_width(n), H.last_chunk_width(n),
                   H.lds_stride(n))
            assert got == TABLE[(d, n)], (d, n, got)
    ds, ns = {d for d, _ in H.ALL_SHAPES}, {n for _, n in H.ALL_SHAPES}
    assert {1, 15} <= ds and all({16 * k - 1, 16 * k, 16 * k + 1} & ds for k in (1, 2, 3, 4))   # panel edges
    assert {15, 16, 17, 33, 48, 49, 64, 65} <= ds
    assert {65, 129, 193} <= ns and {64, 128, 192, 256} <= ns      # one column in the last tile and chunk; full chunks
    # LDS of one block and blocks per CU: 160 KB / ((16 ldx + 256) doubles), at most 16
    assert [H.blocks_per_cu(n) for n in (32, 64, 65, 193, 256)] == [16, 15, 11, 5, 4]
    for d, n in H.STRIDE_SHAPES:
        cus = 256
        batch = 16 * cus + 3
        g = H.grid_of(batch, n, cus)
        assert 8 <= g and g + 1 < batch - 1 and batch > 16 * cus >= g     # a second pass whatever bpc is


def test_lattices_are_seeded_and_all_different():
    seen = set()
    for d, n in H.ALL_SHAPES:
        cases = H.launch(d, n)
        assert len(cases) == H.BATCH and cases[6][1] is cases[0][1]
        fams = [f for f, _ in cases]
        want = {"dense", "qary", "tri"} | ({"zero_row"} if d >= 2 else set())
        assert set(fams) == want, (d, n, fams)
        for L, (fam, b) in enumerate(cases[:6]):
            assert b.shape == (d, n) and b.dtype == np.int64 and not b.flags.writeable
            assert np.array_equal(b, H.GENERATORS[fam](d, n, L))          # seeded
            assert W._key(b) not in seen
            seen.add(W._key(b))
            if fam == "zero_row":
                z = H.zero_row_index(d, n, L)
                assert z < d - 1 and not b[z].any() and all(b[i].any() for i in range(d) if i != z)
                assert z >= 16 or d < 18          # in the second panel where there is one with a successor row
            if fam == "tri":
                assert not np.triu(b, 1).any() and np.all(np.diag(b[:, :d]) != 0)
                assert d < 3 or (np.diag(b[:, :d])[2::3] < 0).all() and (np.diag(b[:, :d])[0::3] > 0).all()
        if d * n >= 15 * 15:
            mags = sorted(float(np.abs(b).max()) for f, b in cases[:6] if f in ("dense", "zero_row"))
            assert mags[-1] > mags[0]             # neighbours of different magnitude in one launch


@pytest.mark.parametrize("shape", H.ALL_SHAPES, ids=_sid)
def test_oracle_is_within_the_cap_of_the_true_factor(shape):
    """the condition on the inputs: oracle (= exact mode) error <= 2^-44 of the row norm, both row_expo settings; the
    exact families' answers ride along"""
    d, n = shape
    worst = 0.0
    for L, (fam, b) in enumerate(H.launch(d, n)[:6]):
        for row_expo in (True, False):
            R, V, sg, e = C.oracle_hh_update_all(b, row_expo)
            assert np.all(np.isfinite(R)) and np.all(np.isfinite(V)) and np.all(np.diag(R[:, :d]) >= 0)
            if not row_expo:
                assert not e.any()
            if fam == "tri":
                assert np.array_equal(H.scaled_tril(R, e), H.tri_expected(b)), (L, row_expo)
                assert not V.any() and np.array_equal(sg, np.where(np.diag(b[:, :d]) < 0, -1.0, 1.0))
                continue
            if fam == "zero_row":
                z = H.zero_row_index(d, n, L)
                assert not R[z].any() and e[z] == 0 and sg[z] == 1.0 and not V[z].any()
            err = H.factor_error(b, R, e)
            assert err <= CAP, (L, fam, row_expo, W.log2(err))
            if d == 1:
                # R(0,0) = sqrt(x_0^2 + sum of the tail's squares): exact at n = 1, a few roundings of 2^-53 at n = 5
                # (2^-53.5 here; seeds 0 .. 11 give 2^-52.4 .. 2^-53.9) — below the floor of the gate, which decides
                assert err == 0 if n == 1 else err < H.GATE_FLOOR
            worst = max(worst, float(err))
    C.note(lambda: ("oracle vs true factor %s: 2^%.1f" % (_sid(shape), np.log2(worst) if worst else -np.inf),))


@pytest.mark.parametrize("shape", [(17, 17), (33, 40), (17, 65)], ids=_sid)
def test_zero_row_true_factor_is_a_factor_of_the_gram_matrix(shape):
    """hh_cases._zero_row_factor on its own: L is lower triangular with a positive diagonal but for row z = 0, L L^T is
    the Gram matrix to 280 bits, the rows before z are the Cholesky rows of those rows alone, and column z is not 0 (the
    coordinate a skipped reflector leaves behind: the factor of the lattice WITHOUT the row would have no such column)"""
    d, n = shape
    L3 = next(L for L in range(6) if H.family_of(d, n, L) == "zero_row")
    b = H.launch(d, n)[L3][1]
    z = H.zero_row_index(d, n, L3)
    Lf = H.true_factor(b)
    mp = F.mp
    old = mp.mp.prec
    mp.mp.prec = H.PREC
    try:
        assert all(len(Lf[i]) == i + 1 for i in range(d)) and all(Lf[i][i] > 0 for i in range(d) if i != z)
        assert not any(Lf[z])
        G = W._matmul_exact(b.astype(object), b.astype(object).T)
        for i in range(d):
            for j in range(i + 1):
                got = mp.fdot(Lf[i][:j + 1], Lf[j][:j + 1])
                assert abs(got - int(G[i][j])) <= mp.ldexp(abs(int(G[i][i])) + 1, -280), (i, j)
        head = W.cholesky(b[:z]) if z else []
        for i in range(z):
            assert max(abs(x - y) for x, y in zip(Lf[i], head[i])) <= mp.ldexp(Lf[i][i], -280)
        assert any(Lf[i][z] != 0 for i in range(z + 1, d))
    finally:
        mp.mp.prec = old


@pytest.mark.parametrize("shape", [(16, 16), (33, 40), (17, 65)], ids=_sid)
def test_the_checker_rejects_doctored_results(shape):
    d, n = shape
    cases = H.launch(d, n)
    out = {}
    for L, (fam, b) in enumerate(cases[:6]):
        R, _, _, e = C.oracle_hh_update_all(b, True)
        out[L] = (R, e)
    for L, (fam, b) in enumerate(cases[:6]):
        R, e = out[L]
        if fam == "tri":
            # exact family: one ulp anywhere is caught
            bad = R.copy()
            bad[d - 1, 0] = np.nextafter(bad[d - 1, 0], np.inf)
            assert not np.array_equal(H.scaled_tril(bad, e), H.tri_expected(b))
            continue
        err = H.factor_error(b, R, e)
        gate = H.gate(err)
        assert err <= gate <= 2.0 ** -40
        # (a) one entry moved by 2^-40 of its row norm
        i = d - 1 if b[d - 1].any() else d - 2
        rown = float(np.sqrt((b[i].astype(np.float64) ** 2).sum()))
        for j in (0, i):
            bad = R.copy()
            bad[i, j] += np.ldexp(rown * 2.0 ** -40, -int(e[i]))
            assert H.factor_error(b, bad, e) > gate, (L, fam, j)
        # (b) another lattice's R in its place
        other = next(M for M in range(6) if M != L and cases[M][0] != "tri")
        assert H.factor_error(b, out[other][0], out[other][1]) > gate
        # (c) one row's exponent off by one
        for step in (1, -1):
            e2 = e.copy()
            e2[i] += step
            assert H.factor_error(b, R, e2) > 2.0 ** -8 > gate
        if fam == "zero_row":
            z = H.zero_row_index(d, n, L)
            bad = R.copy()
            bad[z, 0] = 5e-324
            assert H.factor_error(b, bad, e) == F.mp.inf


def test_grid_stride_plan_and_the_last_row_shortcut():
    """stride_plan: all lattices distinct but g, g + 1 = 0, 1; a wave meets another base on its second pass; and the
    shortcut the GPU test uses for ~4 100 lattices — rows 0 .. d-2 of R do not depend on the last row of the basis (bit
    for bit in the oracle), the last row of the true factor from last_row_factor equals the full Cholesky's"""
    cus = 256
    for d, n in H.STRIDE_SHAPES:
        batch = 16 * cus + 3
        g = H.grid_of(batch, n, cus)
        bs, base, add = H.stride_batch(d, n, batch, g)
        assert bs.shape == (batch, d, n) and list(base[:8]) == list(range(8)) and list(add[:8]) == list(range(8))
        keys = {}
        for L in range(batch):
            keys.setdefault((int(base[L]), int(add[L])), []).append(L)
        assert sorted(v for v in keys.values() if len(v) > 1) == [[0, g], [1, g + 1]]
        assert np.array_equal(bs[g], bs[0]) and np.array_equal(bs[g + 1], bs[1])
        later = np.arange(g + 2, batch)
        assert np.all(base[later] != base[later - g])            # stale LDS would hold ANOTHER base's reflectors
        for L in (5, g - 1, g + 2, batch - 1):
            k = int(base[L])
            b0 = H.stride_base(d, n, k)
            assert np.array_equal(bs[L][:d - 1], b0[:d - 1]) and bs[L][d - 1, n - 1] == b0[d - 1, n - 1] + L
            for row_expo in (True, False):
                R0, _, _, e0 = C.oracle_hh_update_all(b0, row_expo)
                R1, _, _, e1 = C.oracle_hh_update_all(bs[L], row_expo)
                assert np.array_equal(R0[:d - 1].view(np.uint64), R1[:d - 1].view(np.uint64))
                assert np.array_equal(e0[:d - 1], e1[:d - 1]) and not np.array_equal(R0[d - 1], R1[d - 1])
            row, rown = H.last_row_factor(b0, H.true_factor(b0), H.gram_last_row(b0), int(add[L]))
            full = W.cholesky(bs[L])
            mp = F.mp
            old = mp.mp.prec
            mp.mp.prec = H.PREC
            try:
                assert max(abs(x - y) for x, y in zip(row, full[d - 1])) <= mp.ldexp(rown, -280)
                assert abs(rown - mp.sqrt(mp.fsum(t * t for t in full[d - 1]))) <= mp.ldexp(rown, -280)
            finally:
                mp.mp.prec = old
            R1, _, _, e1 = C.oracle_hh_update_all(bs[L], True)
            whole = float(W.r_factor_error(bs[L], (R1,), e1))
            rows = max(H.row_error(full[i], mp.sqrt(mp.fsum(t * t for t in full[i])), R1[i, :i + 1], e1[i])
                       for i in range(d))
            assert abs(rows - whole) <= 1e-12 * whole            # row_error is r_factor_error, row by row


def test_reduced_bases_meet_the_stated_tolerance_in_the_reference_arithmetic():
    """the README's "1e-9 on mu / r" against the EXACT Gram-Schmidt: the oracle's R on the smallest of the reduced bases
    the GPU test uses (the others take seconds of Cholesky and are left to it)"""
    b = H.reduced_base("q48")
    R, _, _, e = C.oracle_hh_update_all(b, True)
    assert H.mu_r_violations(b, R, e) == (0, 0)
    bad = R.copy()
    bad[40, 3] += np.ldexp(4e-9 * np.ldexp(R[3, 3], int(e[3])), -int(e[40]))      # mu(40,3) off by 4e-9
    assert H.mu_r_violations(b, bad, e) != (0, 0)
