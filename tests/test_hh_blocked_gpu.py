"""hh_blocked_kernel<NQ> (fphip_hh_update_R_blocked, MatHouseholderBatch.update_R(blocked=True)) — the compact-WY
R-factor on the matrix cores — against the TRUE R-factor at 300 bits, at every NQ and every panel / tile edge, with
different lattices in every launch (tests/hh_cases.py; its properties are shown on the CPU in tests/test_hh_cases_cpu.py).

The gate: err = worst |R(i,j) 2^row_expo[i] - L(i,j)| / |b_i| over j <= i, L the true factor;
    err(blocked) <= 2^4 max(err(exact mode, same lattice), 2^-52)
— 4 bits for "the same recurrence summed in another order" (DESIGN 4d), the floor one ulp of an entry the size of the
row norm.  The exact mode is first shown to BE the reference arithmetic (the C oracle's bits), so the gate is measured
against the reference, never against the kernel under test.  `tri` lattices must come out exactly."""
import functools
import subprocess
import sys

import numpy as np
import pytest

import conftest as C
import hh_cases as H
import wide_cases as W

pytestmark = pytest.mark.gpu

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _handle(ctx, bs, row_expo):
    from fplll_amd.householder import MatHouseholderBatch
    h = MatHouseholderBatch(ctx, len(bs), bs[0].shape[0], bs[0].shape[1], row_expo=row_expo)
    h.set_basis(np.stack(bs) if isinstance(bs, list) else bs)
    return h


def _read(h):
    out = [h.get_R(L) for L in range(h.batch)]
    return np.stack([R for R, _ in out]), np.stack([e for _, e in out])


@functools.lru_cache(maxsize=None)
def _cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process of its own: in this one the
    library's HIP runtime is already up (the session's Context), and torch does not find the device after it"""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    return int(out.split()[-1])


def _lg(x):
    return W.log2(x) if x else float("-inf")


@pytest.mark.parametrize("row_expo", [True, False], ids=["expo1", "expo0"])
@pytest.mark.parametrize("shape", H.ALL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_blocked_R_against_the_true_factor(ctx, shape, row_expo):
    """One launch of seven lattices (hh_cases.launch: six different ones of four families, the first again at index 6):
    status, row exponents = the exact mode's = the oracle's, diag(R) >= 0; the exact mode returns the oracle's bits; the
    gate of the module docstring on every lattice; `tri` exactly, the zero row exactly 0; the same bits at index 6, on a
    second call and on a fresh handle that never ran the exact mode."""
    d, n = shape
    cases = H.launch(d, n)
    bs = [b for _, b in cases]
    h = _handle(ctx, bs, row_expo)
    assert list(h.update_R()) == [1] * H.BATCH
    Re, ee = _read(h)
    assert list(h.update_R(blocked=True)) == [1] * H.BATCH
    ms = h.last_kernel_ms
    Rb, eb = _read(h)
    assert list(h.update_R(blocked=True)) == [1] * H.BATCH
    Rb2, eb2 = _read(h)
    h.close()
    h = _handle(ctx, bs, row_expo)                      # never ran the exact mode: V, sigma, R, row_expo are shared
    assert list(h.update_R(blocked=True)) == [1] * H.BATCH
    Rb3, eb3 = _read(h)
    h.close()
    # determinism: the same bits again, on a fresh handle, and at index 6 = index 0
    assert np.array_equal(_bits(Rb2), _bits(Rb)) and np.array_equal(eb2, eb)
    assert np.array_equal(_bits(Rb3), _bits(Rb)) and np.array_equal(eb3, eb)
    assert np.array_equal(_bits(Rb[6]), _bits(Rb[0])) and np.array_equal(_bits(Re[6]), _bits(Re[0]))
    worst_e = worst_b = 0
    for L, (fam, b) in enumerate(cases):
        Ro, _, _, eo = C.oracle_hh_update_all(b, row_expo)
        assert np.array_equal(ee[L], eo) and np.array_equal(eb[L], eo), (L, fam)
        assert np.array_equal(_bits(np.tril(Re[L][:, :d])), _bits(np.tril(Ro[:, :d]))), (L, fam)
        assert np.all(np.isfinite(Rb[L])) and np.all(np.diag(Rb[L][:, :d]) >= 0), (L, fam)
        if fam == "tri":
            assert np.array_equal(H.scaled_tril(Rb[L], eb[L]), H.tri_expected(b)), (L, "tri")
            continue
        if fam == "zero_row":
            z = H.zero_row_index(d, n, L)
            assert not Rb[L][z].any() and eb[L][z] == 0, (L, z)
        err_e, err_b = H.factor_error(b, Re[L], ee[L]), H.factor_error(b, Rb[L], eb[L])
        print("  lattice %d %-8s exact mode 2^%.1f blocked 2^%.1f" % (L, fam, _lg(err_e), _lg(err_b)))
        assert err_b <= H.gate(err_e), (L, fam, _lg(err_e), _lg(err_b))
        worst_e, worst_b = max(worst_e, err_e), max(worst_b, err_b)
    C.note(lambda: ("hh_blocked<%d> %dx%d row_expo=%d: exact mode 2^%.1f, blocked 2^%.1f of the row norm; kernel %.3f ms"
                    % (H.nq_of(n), d, n, row_expo, _lg(worst_e), _lg(worst_b), ms),))


@pytest.mark.parametrize("d,n,row_expo", [H.STRIDE_SHAPES[0] + (True,), H.STRIDE_SHAPES[1] + (False,)],
                         ids=lambda v: str(int(v)))
def test_grid_stride_loop_second_pass_over_stale_lds(ctx, d, n, row_expo):
    """More lattices than the grid has waves (16 CUs' worth + 3 > CUs x bpc for any bpc): every wave takes a second
    lattice with the previous one's panel and T still in LDS.  All ~4 100 lattices are different (8 bases in turn, one
    further on each pass, the lattice's index added at (d-1, n-1)) but g, g+1 = 0, 1, g the grid.  Rows 0 .. d-2 of R
    depend on the base alone — the same bits as the base's first lattice, in both modes, whose whole-factor errors are
    measured — and the last row, the one that goes through the matrix cores, is measured against the true factor on
    EVERY lattice (hh_cases.last_row_factor); six lattices are checked from scratch as well."""
    cus = _cu_count()
    batch = 16 * cus + 3
    g = H.grid_of(batch, n, cus)
    assert 8 <= g and g + 1 < batch - 1
    bs, base, add = H.stride_batch(d, n, batch, g)
    h = _handle(ctx, bs, row_expo)
    assert int(h.update_R().min()) == 1
    Re, ee = _read(h)
    assert int(h.update_R(blocked=True).min()) == 1
    ms = h.last_kernel_ms
    Rb, eb = _read(h)
    h.close()
    assert np.array_equal(eb, ee) and np.all(np.isfinite(Rb))
    assert np.all(Rb[:, np.arange(d), np.arange(d)] >= 0)
    # the same input on a first and on a second pass
    for r in (0, 1):
        assert np.array_equal(_bits(Rb[g + r]), _bits(Rb[r])), r
    # rows 0 .. d-2: the base's, bit for bit (lattices 0 .. 7 are the bases' first)
    for R, e in ((Re, ee), (Rb, eb)):
        first = np.tril(R[:, :d - 1, :d])
        bad = np.nonzero((_bits(first) != _bits(first[base])).any(axis=(1, 2)) | (e[:, :d - 1] != e[base][:, :d - 1]).any(axis=1))[0]
        assert bad.size == 0, (bad[:8], g)
    # whole-factor error of those rows per base and mode, last row per lattice
    head = np.zeros((H.STRIDE_BASES, 2))
    facs = []
    for k in range(H.STRIDE_BASES):
        b0 = H.stride_base(d, n, k)
        Lf = H.true_factor(b0)
        norms = [float(np.sqrt(float(sum(int(v) * int(v) for v in b0[i])))) for i in range(d)]
        for m, (R, e) in enumerate(((Re, ee), (Rb, eb))):
            head[k, m] = max(H.row_error(Lf[i], norms[i], R[k][i, :i + 1], e[k][i]) for i in range(d - 1))
        facs.append((b0, Lf, H.gram_last_row(b0)))
    worst = np.zeros(2)
    for L in range(batch):
        k = int(base[L])
        row, rown = H.last_row_factor(*facs[k], int(add[L]))
        err_e = max(head[k, 0], H.row_error(row, rown, Re[L][d - 1, :d], ee[L][d - 1]))
        err_b = max(head[k, 1], H.row_error(row, rown, Rb[L][d - 1, :d], eb[L][d - 1]))
        assert err_b <= 2 ** H.GATE_BITS * max(err_e, H.GATE_FLOOR), (L, k, g, np.log2(err_e), np.log2(err_b))
        worst = np.maximum(worst, (err_e, err_b))
    # from scratch: the oracle's bits in the exact mode, the gate on the whole factor
    for L in (0, 1, g - 1, g, g + 1, batch - 1):
        Ro, _, _, eo = C.oracle_hh_update_all(bs[L], row_expo)
        assert np.array_equal(ee[L], eo)
        assert np.array_equal(_bits(np.tril(Re[L][:, :d])), _bits(np.tril(Ro[:, :d]))), L
        err_e, err_b = H.factor_error(bs[L], Re[L], ee[L]), H.factor_error(bs[L], Rb[L], eb[L])
        assert err_b <= H.gate(err_e), (L, _lg(err_e), _lg(err_b))
    C.note(lambda: ("hh_blocked<%d> grid stride %dx%d row_expo=%d: batch %d on a grid of %d (%d CUs x %d): exact mode 2^%.1f, "
                    "blocked 2^%.1f; kernel %.2f ms" % (H.nq_of(n), d, n, row_expo, batch, g, cus, H.blocks_per_cu(n),
                                                        np.log2(worst[0]), np.log2(worst[1]), ms),))


@pytest.mark.parametrize("src", H.REDUCED)
def test_blocked_mu_and_r_on_reduced_bases_against_exact_gram_schmidt(ctx, src):
    """The stated tolerance of the blocked mode — 1e-9 max(1, |mu|) on mu = R_ij / R_jj, 1e-9 max(|r|, R_ii R_jj) on
    r = R_ij R_jj — on the reduced bases of test_blocked_mfma_mode_agrees_with_exact_mode, with the exact Gram-Schmidt
    (300-bit Cholesky factor) on the other side instead of the exact-mode kernel; the reduced basis is one lattice among
    five different perturbations of itself."""
    bs = H.reduced_launch(src)
    b = bs[H.REDUCED_AT]
    for row_expo in (True, False):
        h = _handle(ctx, bs, row_expo)
        assert list(h.update_R(blocked=True)) == [1] * len(bs)
        Rb, eb = h.get_R(H.REDUCED_AT)
        assert list(h.update_R()) == [1] * len(bs)
        Re, ee = h.get_R(H.REDUCED_AT)
        h.close()
        assert np.array_equal(eb, ee) and np.all(np.diag(Rb[:, :b.shape[0]]) > 0)
        assert H.mu_r_violations(b, Re, ee, src) == (0, 0), "the exact mode itself misses 1e-9 here"
        assert H.mu_r_violations(b, Rb, eb, src) == (0, 0), (src, row_expo)
