"""The transformation matrix u through the device BKZ entry points (FPHIP_BKZ_TRANSFORM: bkz_kernel_u, bkzs_kernel_u,
bkzd_kernel_u).  Every case is a batch of two: lattice 0 starts from u = identity, lattice 1 from u0 = identity +
strictly upper random in [-3, 3] (as test_lll_gpu.py does for LLL).  In exact Python integers:

  * basis, status, tours, node count and enumeration calls are those of the twin run WITHOUT u (and the basis, status
    and node count those of the reference's fixture): tracking u changes nothing else;
  * u[0] b_in = b_out — the inputs have full row rank (checked once, on the CPU, by an exact determinant), so this
    determines u[0] entry by entry and no recorded u is needed;
  * u[1] = u[0] u0[1].

The model of what the kernels do to u in the insertions is the numpy replay of tests/test_bkz_transform_cpu.py."""
import functools
import os

import numpy as np
import pytest

import conftest as C
import wide_cases as W

pytestmark = pytest.mark.gpu

KINDS = ("rotate-only", "unit coefficient", "primal gcd tree", "dual post-processing", "rerandomisation row operations")

# name -> (entry point, extra keyword arguments)
CASES = {
    "bkz_r30_b8": ("bkz", {}),
    "bkz_q40_b10": ("bkz", {}),
    "bkz_u24_hkz": ("bkz", {}),                      # block = d: one hkz
    "bkz_q72_b12_loops2": ("bkz", {}),               # NQ 2, RED_BKZ_LOOPS_LIMIT
    "bkz_q60_b16_autoabort": ("bkz", {}),            # one tour per launch: the u / u2 swap, the inactive-lattice copy
    "bkzs_q50_b20_teststrat_linear": ("bkzs", {}),   # preprocessing tours, pruning
    "bkzs_r40_b32_rerand": ("bkzs", {}),             # rerandomize_block
    "bkzd_q40_b10_sd_loops3": ("bkzs", {"sd": True}),      # dual insertion
    "bkzd_q40_b10_slide": ("bkzs", {"slide": True}),       # BKZ_SLD_RED through bkz_strategies
    "bkzd_r30_b8_slide": ("bkzs", {"slide": True}),
    "hkz14_no_unit_coefficient": ("bkz", {}),        # the primal gcd tree (see NO_UNIT_14)
}

# No committed fixture reaches svp_postprocessing_generic (bkz.cpp:205-272): in ~2000 insertions of the cases above
# every shortest vector has a coefficient +-1.  This 14-dimensional LLL-reduced basis (delta 0.99: lll() leaves it
# as it is) has the shortest vector  -2 b0 + 5 b1 - 4 b2 + 3 b3 + 2 b5 - 2 b7 - 3 b8 - 2 b9 + 2 b11 + 2 b12  of
# squared norm 245258 against |b0|^2 = 10^6, so BKZ-14 (one hkz) inserts it through the gcd tree first thing.
# Found on the CPU: Gram-Schmidt profiles at the edge of what LLL allows (r_ii ~ 0.75^i, mu = +-1/2) as
# lower-triangular integer bases, the block's shortest vector from the C oracle's enumeration, and a hill climb on
# single mu entries towards fewer +-1 coefficients.  Reference for the run: the C oracle's BKZReduction::bkz.
NO_UNIT_14 = np.array([
    [1000, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [491, 872, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [-13, 427, 761, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [-304, -430, 379, 663, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [-495, 432, 382, 327, 578, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [504, 437, 387, -331, 292, 505, 0, 0, 0, 0, 0, 0, 0, 0],
    [-500, -438, 375, 338, -288, 253, 440, 0, 0, 0, 0, 0, 0, 0],
    [-493, 431, -374, -338, 288, 249, -220, 384, 0, 0, 0, 0, 0, 0],
    [200, -434, -371, -1, -7, -5, -219, -189, 335, 0, 0, 0, 0, 0],
    [-507, 443, 385, 327, 293, 251, 216, -192, -170, 292, 0, 0, 0, 0],
    [-300, -433, -386, -335, 288, 248, 216, -195, -166, -144, 255, 0, 0, 0],
    [-499, -438, -378, -332, 291, -251, -220, 194, 170, 148, -129, 222, 0, 0],
    [-504, -440, 373, -335, -3, 257, -134, -191, 167, 148, 129, -109, 194, 0],
    [491, 265, 383, 338, -294, 253, 221, 191, -169, 146, -125, 113, -96, 169]], dtype=np.int64)
NO_UNIT_14_X = (-2, 5, -4, 3, 0, 2, 0, -2, -3, -2, 0, 2, 2, 0)


def _u0(d):
    rng = np.random.default_rng(5)
    return np.stack([np.eye(d, dtype=np.int64), np.triu(rng.integers(-3, 4, size=(d, d)), 1) + np.eye(d, dtype=np.int64)])


def _obj(a):
    return np.asarray(a).astype(object)


def _nodes(info_row):
    return (int(info_row[1]) & 0xffffffff) | ((int(info_row[2]) & 0xffffffff) << 32)


@functools.lru_cache(maxsize=None)
def _full_row_rank(key):
    b = W._unkey(key)
    gram = _obj(b).dot(_obj(b).T)   # (d x d: positive determinant exactly when the d rows are independent)
    return W.bareiss_det(gram) > 0


def full_row_rank(b):
    return _full_row_rank(W._key(b))


def _qary(rng, d, k, q):
    b = np.zeros((d, d), dtype=np.int64)
    b[:k, :k] = np.eye(k, dtype=np.int64)
    b[:k, k:] = rng.integers(0, q, size=(k, d - k))
    b[k:, k:] = q * np.eye(d - k, dtype=np.int64)
    return b


def _call(g, f, kind, kw, transform, batch):
    """the fixture's BKZ call on g; returns (status, info, keep-alive)"""
    if kind == "bkz":
        return g.bkz(f["block_size"], f["delta"], f["eta"], f["max_loops"], f["auto_abort"], transform=transform) + (None,)
    S = f.get("strategies")
    rnd, draws = C.gmp_streams_native(batch, f["rng_seed"]) if S is not None else (None, None)
    st, info = g.bkz_strategies(f["block_size"], S, rnd, f["delta"], f["eta"], max_loops=f["max_loops"],
                                gh_bnd=bool(f["flags"] & 0x80), bounded_lll=bool(f["flags"] & 0x10),
                                gh_factor=f["gh_factor"], auto_abort=bool(f["flags"] & 0x20), transform=transform, **kw)
    return st, info, rnd


def _no_unit_case():
    """NO_UNIT_14 under BKZ-14 in the form of a fixture, the expected values from the C oracle"""
    o = C.OracleGSO(NO_UNIT_14)
    st, info = o.bkz(14)
    f = dict(d=14, n=14, block_size=14, delta=0.99, eta=0.51, max_loops=0, auto_abort=False, b_in=NO_UNIT_14,
             status=int(st), nodes=_nodes(info), b_out=o.b.copy())
    o.close()
    # the inserted vector is the one announced above
    assert np.array_equal(_obj(f["b_out"][0]), np.array(NO_UNIT_14_X, dtype=object).dot(_obj(NO_UNIT_14)))
    return f


_RESULTS = {}


def run_case(ctx, name):
    """the case's run with u and its twin without, once per session: dict(f, b_in[2], u0, st, info, out, u, stats, and
    the twin's st_t, info_t, out_t)"""
    if name in _RESULTS:
        return _RESULTS[name]
    from fplll_amd.gso import MatGSOBatch
    kind, kw = CASES[name]
    f = _no_unit_case() if name == "hkz14_no_unit_coefficient" else C.load_bkz_fixture(os.path.join(C.GOLDEN, name + ".json"))
    b1 = _second_lattice(ctx, name)
    b_in = np.stack([f["b_in"], f["b_in"] if b1 is None else b1])
    u0 = _u0(f["d"])
    r = dict(f=f, b_in=b_in, u0=u0, same_input=b1 is None)
    g = MatGSOBatch(ctx, 2, f["d"], f["n"])
    g.set_basis(b_in)
    r["st_t"], r["info_t"], _keep = _call(g, f, kind, kw, False, 2)
    r["out_t"] = g.get_basis()
    g.close()
    g = MatGSOBatch(ctx, 2, f["d"], f["n"])
    g.set_basis(b_in)
    g.enable_transform(u0)
    r["st"], r["info"], _keep = _call(g, f, kind, kw, True, 2)
    r["out"], r["u"], r["stats"] = g.get_basis(), g.get_transform(), g.bkz_insert_stats()
    r["ms"] = g.last_kernel_ms
    g.close()
    _RESULTS[name] = r
    return r


def check_algebra(b_in, b_out, u, u0, lattice1_same_input=True):
    """u[0] b_in[0] = b_out[0]; lattice 1: u[1] = u[0] u0[1] when it holds the same input, u[1] = T u0[1] with
    T b_in[1] = b_out[1] otherwise (T from the exact inverse of u0[1])."""
    assert full_row_rank(b_in[0])
    assert np.array_equal(_obj(u[0]).dot(_obj(b_in[0])), _obj(b_out[0]))
    if lattice1_same_input:
        assert np.array_equal(b_out[1], b_out[0])
        assert np.array_equal(_obj(u[1]), _obj(u[0]).dot(_obj(u0[1])))
    else:
        from fplll_amd.gso import inverse_transpose
        assert full_row_rank(b_in[1])
        t = _obj(u[1]).dot(inverse_transpose(u0[1]).T)
        assert np.array_equal(t.dot(_obj(b_in[1])), _obj(b_out[1]))


def _second_lattice(ctx, name):
    """bkz_q60_b16_autoabort: lattice 1 is ANOTHER (LLL-reduced) q-ary basis, so that the two reductions end after a
    different number of one-tour launches and the finished one is copied through (b and u) by the later ones.
    (Found with the CPU oracle: this one takes 14 tours under BKZ-16 with auto-abort, the fixture's lattice 17 — the
    lattice that starts from u0 is the one that waits; the test asserts that the counts differ.)"""
    if name != "bkz_q60_b16_autoabort":
        return None
    from fplll_amd.gso import MatGSOBatch
    rng = np.random.default_rng(2025)
    g = MatGSOBatch(ctx, 1, 60, 60)
    g.set_basis(_qary(rng, 60, 20, 257)[None])
    st, _ = g.lll()
    assert list(st) == [1]
    b1 = g.get_basis()[0]
    g.close()
    return b1


@pytest.mark.parametrize("name", list(CASES))
def test_u_follows_the_bkz_run(ctx, name):
    r = run_case(ctx, name)
    f = r["f"]
    C.note(lambda: ("%s: status %s tours %s nodes %s calls %s, insertions by kind %s, kernel %.1f ms"
                    % (name, list(r["st"]), list(r["info"][:, 0]), [_nodes(i) for i in r["info"]], list(r["info"][:, 3]),
                       dict(zip(KINDS, r["stats"])), r["ms"]),))
    # the run with u is the run without: the fixture's basis, status and node count, the twin's tours and calls
    assert r["st"][0] == f["status"] and _nodes(r["info"][0]) == f["nodes"]
    assert np.array_equal(r["out"][0], f["b_out"])
    assert np.array_equal(r["st"], r["st_t"]) and np.array_equal(r["info"], r["info_t"])
    assert np.array_equal(r["out"], r["out_t"])
    check_algebra(r["b_in"], r["out"], r["u"], r["u0"], lattice1_same_input=r["same_input"])
    if not r["same_input"]:
        assert int(r["info"][0][0]) != int(r["info"][1][0]), "the two lattices were meant to end after different tours"
    assert sum(r["stats"]) > 0
    if name == "hkz14_no_unit_coefficient":
        assert r["stats"][2] > 0


def test_every_kind_of_insertion_was_exercised(ctx):
    """fphip_gso_bkz_insert_stats summed over the cases above: each of the five places where the kernels act on u
    outside LLL has run, so the algebra checks above cover it."""
    total = [0] * 5
    for name in CASES:
        r = run_case(ctx, name)
        total = [a + int(b) for a, b in zip(total, r["stats"])]
    C.note(lambda: ("insertions by kind over all cases", dict(zip(KINDS, total)),))
    for kind, count in zip(KINDS, total):
        assert count > 0, kind
    # a run without the flag leaves the counters at zero
    from fplll_amd.gso import MatGSOBatch
    f = C.load_bkz_fixture(os.path.join(C.GOLDEN, "bkz_r30_b8.json"))
    g = MatGSOBatch(ctx, 1, f["d"], f["n"])
    g.set_basis(f["b_in"][None])
    g.bkz(f["block_size"], f["delta"], f["eta"])
    assert g.bkz_insert_stats() == (0, 0, 0, 0, 0)
    g.close()


def test_handoff_blocks_keep_u_in_step(ctx, monkeypatch):
    """FPHIP_BKZ_HANDOFF, forced as test_bkzs_gpu.py forces it: the vector comes from the multi-wave enumerator
    (another visiting order: no golden basis), the insertion still happens in the kernel — the algebra holds."""
    from fplll_amd.gso import MatGSOBatch
    f = C.load_bkz_fixture(os.path.join(C.GOLDEN, "bkzs_r40_b32_rerand.json"))
    monkeypatch.setenv("FPHIP_BKZ_HANDOFF_NODES", "200")
    monkeypatch.setenv("FPHIP_BKZ_HANDOFF_WORKERS", "2")
    b_in = np.stack([f["b_in"]] * 2)
    u0 = _u0(f["d"])
    g = MatGSOBatch(ctx, 2, f["d"], f["n"])
    g.set_basis(b_in)
    g.enable_transform(u0)
    st, info, _keep = _call(g, f, "bkzs", {"handoff": True}, True, 2)
    out, u = g.get_basis(), g.get_transform()
    g.close()
    assert list(st) == [f["status"]] * 2
    # (a parallel enumeration is order dependent, the two tours may differ: each lattice by its own algebra)
    check_algebra(b_in, out, u, u0, lattice1_same_input=False)


def test_wide_basis_three_chunks(ctx):
    """40 x 129 (NQ 3: u has one chunk in use, b three): LLL then BKZ-12 on one object, u through both; against the
    twin without u and by the algebra on the ORIGINAL basis."""
    from fplll_amd.gso import MatGSOBatch
    d, n = W.SHORT_WIDE_BKZ[0]
    assert (d, n) == (40, 129) and W.nq_of(d, n) == 3
    b = W.short_wide(d, n, 0)
    b_in = np.stack([b, b])
    u0 = _u0(d)
    res = []
    for with_u in (False, True):
        g = MatGSOBatch(ctx, 2, d, n)
        g.set_basis(b_in)
        if with_u:
            g.enable_transform(u0)
        st, _ = g.lll()
        assert list(st) == [1, 1]
        st, info = g.bkz(12, transform=with_u)
        res.append((st, info, g.get_basis(), g.get_transform() if with_u else None))
        g.close()
    (st_t, info_t, out_t, _), (st, info, out, u) = res
    assert list(st) == [1, 1]
    assert np.array_equal(st, st_t) and np.array_equal(info, info_t) and np.array_equal(out, out_t)
    check_algebra(b_in, out, u, u0)


def test_contract(ctx):
    """transform=True needs enable_transform; a tracked u without the flag is refused as before; slide_pass refuses a
    tracked u in any case — and none of the refusals touches b or u."""
    from fplll_amd.gso import MatGSOBatch
    f = C.load_bkz_fixture(os.path.join(C.GOLDEN, "bkzd_q40_b10_slide.json"))
    g = MatGSOBatch(ctx, 1, f["d"], f["n"])
    g.set_basis(f["b_in"][None])
    with pytest.raises(Exception, match="fphip_gso_enable_transform"):
        g.bkz(f["block_size"], f["delta"], f["eta"], transform=True)
    with pytest.raises(Exception, match="fphip_gso_enable_transform"):
        g.bkz_strategies(f["block_size"], None, None, f["delta"], f["eta"], transform=True)
    g.enable_transform()
    with pytest.raises(Exception):
        g.bkz(f["block_size"], f["delta"], f["eta"])
    with pytest.raises(Exception):
        g.bkz_strategies(f["block_size"], None, None, f["delta"], f["eta"])
    with pytest.raises(Exception):
        g.slide_pass(1, 1, f["block_size"])
    assert np.array_equal(g.get_basis()[0], f["b_in"])
    assert np.array_equal(g.get_transform()[0], np.eye(f["d"], dtype=np.int64))
    g.close()


def test_bkz_reduction_chain(ctx):
    """gso.bkz_reduction on an UNREDUCED q-ary basis: u b_orig = b_out, b_out is lll() then bkz() of an object
    without u, and get_inverse_transform_t() of the same chain on an object is the inverse transpose of u."""
    from fplll_amd import gso
    d, beta = 40, 10
    b = _qary(np.random.default_rng(77), d, d // 2, 4099)
    b_out, u, st, info = gso.bkz_reduction(ctx, b, beta)
    assert st == 1 and u.shape == (d, d) and b_out.shape == (d, d)
    assert W.bareiss_det(b) != 0
    assert np.array_equal(_obj(u).dot(_obj(b)), _obj(b_out))
    g = gso.MatGSOBatch(ctx, 1, d, d)
    g.set_basis(b[None])
    assert list(g.lll()[0]) == [1]
    st2, info2 = g.bkz(beta)
    assert st2[0] == st and np.array_equal(info2[0], info)
    assert np.array_equal(g.get_basis()[0], b_out)
    g.close()
    g = gso.MatGSOBatch(ctx, 1, d, d)
    g.set_basis(b[None])
    g.enable_transform()
    g.lll()
    g.bkz(beta, transform=True)
    assert np.array_equal(g.get_transform()[0], u)
    uit = g.get_inverse_transform_t()[0]
    assert np.array_equal(uit.dot(_obj(u).T), _obj(np.eye(d, dtype=np.int64)))
    g.close()
    # a batch, without u
    bb, uu, sts, _ = gso.bkz_reduction(ctx, np.stack([b, b]), beta, with_u=False)
    assert uu is None and list(sts) == [1, 1] and np.array_equal(bb[1], b_out)
