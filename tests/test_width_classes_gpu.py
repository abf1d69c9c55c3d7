"""Every columns-per-lane instantiation (NQ = 2, 3, 4) of the reduction kernels on inputs that need it, against the C
oracle — bit for bit where the kernel keeps the reference's order of operations (lll, hlll(), bkz, bkz_strategies),
against exact arithmetic where it sums in tree order (lll_ex, hlll(precision = p)).  The inputs are those of
tests/wide_cases.py (short-wide: NQ decided by the columns alone, five different lattices per launch, both sides of
128/129 and 192/193; tall: 180 and 200 rows, three different lattices per launch), whose properties
tests/test_wide_cases_cpu.py shows on the CPU.

Not launched here: quad-double (precision 212) with more than 64 rows or columns, in either kernel, and the ladders at
test level 2 on a wide shape — DESIGN.md section 4d, OPEN."""
import time

import numpy as np
import pytest

import conftest as C
import wide_cases as W

pytestmark = pytest.mark.gpu

SHORT = [("short", d, n) for d, n in W.SHORT_WIDE]
SHORT_BKZ = [("short", d, n) for d, n in W.SHORT_WIDE_BKZ]
SHORT_BKZS = [("short", d, n) for d, n in W.SHORT_WIDE_BKZS]
TALL = [("tall", 3), ("tall", 4)]


def _id(case):
    return "%dx%d" % case[1:] if case[0] == "short" else "tall%d" % W.tall_base(case[1]).shape[0]


def _inputs(case):
    return W.short_wide_batch(*case[1:]) if case[0] == "short" else W.tall_batch(case[1])


def _gso(ctx, bs):
    from fplll_amd.gso import MatGSOBatch
    g = MatGSOBatch(ctx, len(bs), *bs[0].shape)
    g.set_basis(np.stack(bs))
    return g


def _hh(ctx, bs):
    from fplll_amd.householder import MatHouseholderBatch
    h = MatHouseholderBatch(ctx, len(bs), *bs[0].shape, row_expo=True)
    h.set_basis(np.stack(bs))
    return h


def _first_bad_row(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if bad.size == 0 else int(bad[0])


# ---- 1. lll_kernel<NQ, false / true> -------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 2, 6], ids=["plain", "early_red", "siegel_early_red"])
@pytest.mark.parametrize("case", SHORT + TALL, ids=_id)
def test_lll_matches_oracle(ctx, case, flags):
    """status, (final kappa, swaps, zero rows) and the basis of every lattice; without flags also mu, r and the row
    exponents the call leaves: the oracle's update_all() of the output"""
    bs = _inputs(case)
    g = _gso(ctx, bs)
    st, info = g.lll(flags=flags)
    out = g.get_basis(0, len(bs))
    for L, b in enumerate(bs):
        ost, oinfo, ob = W.oracle_lll(b, flags)
        assert st[L] == ost == 1, (L, st)
        assert tuple(int(x) for x in info[L][:3]) == oinfo[:3], L
        assert _first_bad_row(out[L], ob) is None, (L, _first_bad_row(out[L], ob))
        if flags == 0:
            o = C.OracleGSO(ob)
            assert o.update_all() == 1
            assert np.array_equal(g.row_expo(L), o.row_expo)
            assert np.array_equal(g.get_mu_matrix(L), o.mu)
            assert np.array_equal(g.get_r_matrix(L), o.r)
            o.close()
    C.note(lambda: ("lll %s NQ %d flags %d: swaps %s, kernel %.1f ms"
                    % (_id(case), W.nq_of(*bs[0].shape), flags, [int(i[1]) for i in info], g.last_kernel_ms),))
    g.close()


# ---- 2. hlll_kernel<NQ> --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHORT + TALL, ids=_id)
def test_hlll_matches_oracle(ctx, case):
    bs = _inputs(case)
    d = bs[0].shape[0]
    h = _hh(ctx, bs)
    st, info = h.hlll()
    out = h.get_basis(0, len(bs))
    for L, b in enumerate(bs):
        ost, oinfo, ob = W.oracle_hlll(b)
        assert st[L] == ost == 1, (L, st)
        assert tuple(int(x) for x in info[L]) == oinfo, L
        assert _first_bad_row(out[L], ob) is None, (L, _first_bad_row(out[L], ob))
        R, e = h.get_R(L)
        Ro, Vo, so, eo = C.oracle_hh_update_all(ob, True)
        assert np.array_equal(e, eo)
        assert np.array_equal(np.tril(R[:, :d]), np.tril(Ro[:, :d]))
    C.note(lambda: ("hlll %s NQ %d: swaps %s, kernel %.1f ms"
                    % (_id(case), W.nq_of(*bs[0].shape), [int(i[0]) for i in info], h.last_kernel_ms),))
    h.close()


# ---- 3. bkz_kernel<NQ> ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHORT_BKZ + TALL, ids=_id)
def test_bkz_matches_oracle(ctx, case):
    """device LLL feeds device BKZ, oracle LLL feeds oracle BKZ: status, tours, nodes, basis"""
    bs = _inputs(case)
    beta, max_loops = (12, 0) if case[0] == "short" else (10, 1)
    g = _gso(ctx, bs)
    st, _ = g.lll()
    assert np.all(st == 1)
    st, info = g.bkz(beta, max_loops=max_loops)
    out = g.get_basis(0, len(bs))
    for L, b in enumerate(bs):
        ost, otours, onodes, ob = W.oracle_bkz(W.oracle_lll(b)[2], beta, max_loops)
        assert st[L] == ost, (L, st)
        assert int(info[L][0]) == otours
        assert W.nodes64(info[L]) == onodes
        assert _first_bad_row(out[L], ob) is None, (L, _first_bad_row(out[L], ob))
    C.note(lambda: ("bkz-%d %s NQ %d: tours %s, nodes %s, kernel %.1f ms" % (
        beta, _id(case), W.nq_of(*bs[0].shape), [int(i[0]) for i in info], [W.nodes64(i) for i in info], g.last_kernel_ms),))
    g.close()


# ---- 4. bkzs_kernel<NQ> --------------------------------------------------------------------------------------------------
BKZS = [(c, w, None) for c in SHORT_BKZS + TALL for w in ("rerand", "pre_gh")] + [(TALL[1], "rerand", "0")]


@pytest.mark.parametrize("case,which,mu_lds", BKZS,
                         ids=["%s-%s%s" % (_id(c), w, "" if m is None else "-mu_global") for c, w, m in BKZS])
def test_bkz_strategies_matches_oracle(ctx, case, which, mu_lds, monkeypatch):
    """one tour with the strategies of bkzs_q64_b40_<which> (BKZ_MAX_LOOPS | BKZ_GH_BND), every lattice with its own
    generator stream: status, nodes, basis.  mu_lds "0": FPHIP_BKZ_MU_LDS=0, the block's mu rows in global memory."""
    if mu_lds is not None:
        monkeypatch.setenv("FPHIP_BKZ_MU_LDS", mu_lds)
    bs = _inputs(case)
    beta, seed = (36 if case[0] == "short" else 30), 17
    want = [W.oracle_bkzs(W.oracle_lll(b)[2], beta, which, seed) for b in bs]
    g = _gso(ctx, bs)
    st, _ = g.lll()
    assert np.all(st == 1)
    rnd, draws = C.gmp_streams_native(len(bs), seed)
    st, info = g.bkz_strategies(beta, W.strategies(which), rnd, max_loops=1, gh_bnd=True)
    out = g.get_basis(0, len(bs))
    C.note(lambda: ("bkz_strategies-%d %s %s NQ %d: nodes %s, rerandomisations (oracle) %s, rng draws %d, kernel %.1f ms" % (
        beta, _id(case), which, W.nq_of(*bs[0].shape), [W.nodes64(i) for i in info], [w[3] for w in want], draws(),
        g.last_kernel_ms),))
    for L in range(len(bs)):
        assert st[L] == want[L][0], (L, st)
        assert W.nodes64(info[L]) == want[L][1], L
        assert _first_bad_row(out[L], want[L][4]) is None, (L, _first_bad_row(out[L], want[L][4]))
    g.close()


# ---- 5. lll_x_kernel<NQ, double / DD>, hlll_x_kernel<NQ, double / DD> -----------------------------------------------------
# The gates of tests/test_dd_gpu.py: relative errors of R (to the row norm), mu (to max(1, |mu|)) and r (to r(i,i)).
GATE = {53: -40, 106: -92}
GAIN = 30   # the 106-bit run is at least 2^30 better than the 53-bit one
# mu and r of the tall bases miss those gates by tens of bits in ANY arithmetic of that width: the recurrence r(i,i) =
# |b_i|^2 - sum mu^2 r cancels most of its leading bits on a reduced 180- / 200-row q-ary basis (the reference's own
# double LLL stops with a Babai failure on other perturbations of the 200-row one).  There the gate is 4 bits above
# what the REFERENCE ARITHMETIC gives on the same bases — wide_cases.reference_gso_error: update_gso_row's recurrence
# in mpmath with every operation rounded to 53 / 106 bits, worst of the three lattices, log2 of (mu, r); `python
# tests/wide_cases.py` recomputes the table (two minutes on a CPU).  The kernel's figures are in DESIGN.md section 4d.
REFERENCE_ARITHMETIC = {"tall180": {53: (-16.2, -15.8), 106: (-69.2, -67.9)},
                        "tall200": {53: (-5.5, -5.4), 106: (-59.6, -59.4)}}
# The 106-bit runs return the basis of the oracle's DOUBLE run on every lattice but one: lll_ex(106) on the first
# 200-row lattice, where double has five bits left (table above) and decides a near-tie the other way.
DD_DIFFERS_FROM_DOUBLE = {("lll_ex", "tall200")}


def _mu_r_gate(case, prec, k):
    ref = REFERENCE_ARITHMETIC.get(_id(case))
    return GATE[prec] if ref is None else ref[prec][k] + 4


def _reduced_same_lattice(case, b_in, b_out, violation, **params):
    tall = case[0] == "tall"
    same = W.same_lattice_square(b_in, b_out) if tall else W.same_lattice(b_in, b_out)
    return same, violation(W.exact_gso(b_out, tall), **params)


@pytest.mark.parametrize("case", SHORT + TALL, ids=_id)
def test_lll_ex_against_exact_arithmetic(ctx, case):
    """lll_ex(53) and lll_ex(106): status 1, the output spans the input's lattice (exact), is LLL-reduced by the
    reference's predicate on its exact Gram-Schmidt (no slack), and the mu / r the kernel ends with are those of the
    OUTPUT basis to the accuracy of the type; the planes the type does not have read as zeros."""
    mp = pytest.importorskip("mpmath")
    bs = _inputs(case)
    g = _gso(ctx, bs)
    g.lll_ex_keep(True)
    worst, equal = {}, {}
    for prec in (53, 106):
        g.set_basis(np.stack(bs))
        st, info = g.lll_ex(prec)
        out = g.get_basis(0, len(bs))
        assert list(st) == [1] * len(bs), (prec, st, info)
        wm = wr = mp.mpf(0)
        t = time.time()
        for L, b in enumerate(bs):
            same, viol = _reduced_same_lattice(case, b, out[L], W.lll_violation, delta=0.99, eta=0.51)
            assert same, (prec, L)
            assert viol is None, (prec, L, viol)
            pm = [g.lll_ex_plane(L, 0, k) for k in range(4)]
            pr = [g.lll_ex_plane(L, 1, k) for k in range(4)]
            for k in range(prec // 53, 4):
                assert not pm[k].any() and not pr[k].any(), (prec, L, k)
            em, er = W.mu_r_error(out[L], pm[:prec // 53], pr[:prec // 53], g.row_expo(L))
            wm, wr = max(wm, em), max(wr, er)
        worst[prec] = (wm, wr)
        equal[prec] = [bool(np.array_equal(out[L], W.oracle_lll(b)[2])) for L, b in enumerate(bs)]
        C.note(lambda: ("lll_ex(%d) %s NQ %d: swaps %s, kernel %.1f ms, checks %.1f s, basis == the oracle's double run: %s"
                        % (prec, _id(case), W.nq_of(*bs[0].shape), [int(i[1]) for i in info], g.last_kernel_ms,
                           time.time() - t, equal[prec]),))
    g.close()
    C.note(lambda: ("lll_ex %s vs exact Gram-Schmidt: mu 2^%.1f / 2^%.1f, r 2^%.1f / 2^%.1f at 53 / 106 bits"
                    % ((_id(case),) + tuple(W.log2(worst[p][k]) for k in (0, 1) for p in (53, 106))),))
    if ("lll_ex", _id(case)) not in DD_DIFFERS_FROM_DOUBLE:
        assert all(equal[106]), equal
    for k in (0, 1):
        for prec in (53, 106):
            assert worst[prec][k] <= mp.mpf(2) ** _mu_r_gate(case, prec, k), (prec, k, W.log2(worst[prec][k]))
        assert worst[106][k] * 2 ** GAIN <= worst[53][k], (k, W.log2(worst[106][k]), W.log2(worst[53][k]))


@pytest.mark.parametrize("case", SHORT + TALL, ids=_id)
def test_hlll_ex_against_exact_arithmetic(ctx, case):
    """hlll(precision = 53) and hlll(precision = 106): status 1, the same lattice (exact), HLLL-reduced by the
    reference's predicate on the exact R-factor with the call's delta / eta / theta, and the R the kernel leaves is the
    R-factor of its OUTPUT to the accuracy of the type; the planes the type does not have read as zeros."""
    mp = pytest.importorskip("mpmath")
    bs = _inputs(case)
    h = _hh(ctx, bs)
    worst, equal = {}, {}
    for prec in (53, 106):
        h.set_basis(np.stack(bs))
        st, info = h.hlll(0.99, 0.51, 0.001, 0.1, precision=prec)
        out = h.get_basis(0, len(bs))
        assert list(st) == [1] * len(bs), (prec, st, info)
        w = mp.mpf(0)
        t = time.time()
        for L, b in enumerate(bs):
            same, viol = _reduced_same_lattice(case, b, out[L], W.hlll_violation, delta=0.99, eta=0.51, theta=0.001)
            assert same, (prec, L)
            assert viol is None, (prec, L, viol)
            pl = [h.get_R_plane(L, k) for k in range(4)]
            for k in range(prec // 53, 4):
                assert not pl[k].any(), (prec, L, k)
            w = max(w, W.r_factor_error(out[L], pl[:prec // 53], h.get_R(L)[1]))
        worst[prec] = w
        equal[prec] = [bool(np.array_equal(out[L], W.oracle_hlll(b)[2])) for L, b in enumerate(bs)]
        C.note(lambda: ("hlll(precision=%d) %s NQ %d: swaps %s, kernel %.1f ms, checks %.1f s, basis == the oracle's double "
                        "run: %s" % (prec, _id(case), W.nq_of(*bs[0].shape), [int(i[0]) for i in info], h.last_kernel_ms,
                                     time.time() - t, equal[prec]),))
    h.close()
    C.note(lambda: ("hlll_ex %s R-factor vs the exact Cholesky factor, relative to the row norm: 2^%.1f / 2^%.1f at 53 / 106 "
                    "bits" % (_id(case), W.log2(worst[53]), W.log2(worst[106])),))
    if ("hlll_ex", _id(case)) not in DD_DIFFERS_FROM_DOUBLE:
        assert all(equal[106]), equal
    for prec in (53, 106):
        assert worst[prec] <= mp.mpf(2) ** GATE[prec], (prec, W.log2(worst[prec]))
    assert worst[106] * 2 ** GAIN <= worst[53], (W.log2(worst[106]), W.log2(worst[53]))


# ---- 6. the blocked mode and the ladders on wide shapes -------------------------------------------------------------------
@pytest.mark.parametrize("case", [("short", 20, 193), ("tall", 3)], ids=_id)
def test_blocked_reflectors_on_wide_shapes(ctx, case, monkeypatch):
    """FPHIP_HLLL_BLOCKED=1 at 53 and 106 bits: the basis and the swap counts of the one-by-one mode"""
    bs = _inputs(case)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("FPHIP_HLLL_BLOCKED", mode)
        h = _hh(ctx, bs)
        for prec in (53, 106):
            h.set_basis(np.stack(bs))
            st, info = h.hlll(precision=prec)
            assert list(st) == [1] * len(bs), (mode, prec, st)
            res[(mode, prec)] = (h.get_basis(0, len(bs)), [int(x[0]) for x in info])
        h.close()
    for prec in (53, 106):
        (b0, s0), (b1, s1) = res[("0", prec)], res[("1", prec)]
        assert np.array_equal(b0, b1), prec
        assert s0 == s1, prec


def test_ladders_on_a_wide_shape(ctx, monkeypatch):
    """lll_ladder and hlll_ladder at test level 1 on 20 x 193 (NQ = 4): the odd lattices go on to the double-double
    stage from the basis the double stage left; every lattice ends on the basis of the plain run.  The ladders send a
    lattice that fails at 106 bits on to quad-double, which must not run at this width (OPEN): the
    double-double stage is first shown to succeed on exactly the bases it will get."""
    bs = W.short_wide_batch(20, 193)
    stages = [53, 106, 53, 106, 53]
    g = _gso(ctx, [W.oracle_lll(b)[2] for b in bs])
    st, info = g.lll_ex(106)
    assert list(st) == [1] * 5, st
    monkeypatch.setenv("FPHIP_LLL_LADDER_TEST", "1")
    g.set_basis(np.stack(bs))
    st, info, stage = g.lll_ladder()
    assert list(st) == [1] * 5 and list(stage) == stages
    out = g.get_basis(0, 5)
    for L, b in enumerate(bs):
        assert np.array_equal(out[L], W.oracle_lll(b)[2]), L
    g.close()
    monkeypatch.setenv("FPHIP_HLLL_LADDER_TEST", "1")
    h = _hh(ctx, bs)
    st, info, stage = h.hlll_ladder()
    assert list(st) == [1] * 5 and list(stage) == stages
    out = h.get_basis(0, 5)
    for L, b in enumerate(bs):
        assert np.array_equal(out[L], W.oracle_hlll(b)[2]), L
    h.close()
