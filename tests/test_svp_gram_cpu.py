"""The N-shortest-vectors solver for quadratic forms (fplll_amd.gram.shortest_vectors_gram,
fphip_gram_shortest_vectors, svp_gram.hip), the CPU half: the exact rational enumeration of a form
(tests/exact_form.py) against the one of a basis (tests/exact_lattice.py), the kernel's model (tests/svp_gram_model.py)
against the basis kernel's model on the same mu / r and against the exact enumeration, the 63-bit rule, the recorded
runs of the reference (tests/golden/svpgram_*.json), the C ABI, and the kernel's registers and scratch use read from the
object build() left behind."""
import ctypes
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

import conftest as C
import exact_form as XF
import exact_lattice as X
import solver_families as F
import svp_best_model as BM
import svp_gram_cases as BIG
import svp_gram_model as GM
import svp_model as M

# the reference's two test forms (its tests/lattices/grammatrix_dimension7 / _dimension4) and the answers it holds
DIM7 = [[3, 1, 1, 1, 1, 1, 2], [1, 3, 1, 1, 1, 1, 2], [1, 1, 3, 1, 1, 1, 2], [1, 1, 1, 3, 1, 1, 2], [1, 1, 1, 1, 3, 1, 2],
        [1, 1, 1, 1, 1, 3, 0], [2, 2, 2, 2, 2, 0, 4]]
DIM7_OUT = [1, 1, 1, 0, 1, -1, -2]

_gso = {}


def gram_of(b):
    return [[sum(int(x) * int(y) for x, y in zip(r, s)) for s in b] for r in b]


def _gso_of(b):
    key = tuple(tuple(r) for r in b)
    if key not in _gso:
        _gso[key] = M.gso_of(b)
    return _gso[key]


def _fixture(name):
    return json.load(open(os.path.join(C.GOLDEN, name)))


def _dim4():
    return _fixture("svpgram_dim4_k8.json")


def _nobasis():
    return json.load(open(os.path.join(C.GOLDEN, "lllgram_form_nobasis.json")))


def _shells(lst):
    out = {}
    for nv, _ in lst:
        out[nv] = out.get(nv, 0) + 2
    return out


# ---- 1. the exact enumeration of a form against the one of a basis --------------------------------------------------
@pytest.mark.parametrize("name", F.names())
def test_exact_form_equals_exact_lattice_on_every_member(name):
    """short_exact_form(B B^T, N) is exact_lattice.short_exact(B, N) as a list, nodes included, at the bound of the
    families' size condition (the shortest row's norm - 1, within NODE_CAP) and at the third distinct norm; d_eff and
    the minimum agree."""
    b = F.basis(name)
    G = gram_of(b)
    rn = [G[i][i] for i in range(len(G))]
    norms3, third = F.norms_exact(name, 3)
    for N in (min(rn) - 1, norms3[2]):
        want, wn = X.short_exact(b, N, max_nodes=2 * F.NODE_CAP)
        got, gn = XF.short_exact_form(G, N, max_nodes=2 * F.NODE_CAP)
        assert got == want and gn == wn, (name, N)
        assert wn <= F.NODE_CAP or N == norms3[2]
    assert [(nv, x) for nv, x in XF.short_exact_form(G, norms3[2])[0]] == third
    ex = F.exact(name)
    assert XF.d_eff_exact_form(G) == ex["d_eff"]
    lam, xs, _ = XF.lambda1_exact_form(G, rows=ex["d_eff"], max_nodes=2 * F.NODE_CAP)
    assert lam == ex["lam1"] and {tuple(x) + (0,) * (len(b) - ex["d_eff"]) for x in xs} <= ex["minimal"]
    # rows / level: the leading form and a pruned tree, against the basis side
    lev = F.pruning_of(name)[:ex["d_eff"]]
    from fractions import Fraction
    levq = [Fraction(v) for v in lev]
    assert XF.short_exact_form(G, ex["N0"], rows=ex["d_eff"], level=levq, max_nodes=2 * F.NODE_CAP) == \
        X.short_exact(b, ex["N0"], rows=ex["d_eff"], level=levq, max_nodes=2 * F.NODE_CAP)


def test_the_references_two_forms_have_their_known_shells():
    lst, _ = XF.short_exact_form(DIM7, 4)
    assert _shells(lst) == {3: 56, 4: 126}
    assert XF.sqnorm(DIM7, DIM7_OUT) == 3
    f4 = _dim4()
    lst, _ = XF.short_exact_form(f4["G_in"], 4)
    assert _shells(lst) == {2: 24, 4: 24}
    assert XF.sqnorm(f4["G_in"], f4["ref_out"]) == 2
    assert _fixture("svpgram_dim7_k8.json")["G_in"] == DIM7 and _fixture("svpgram_dim7_k8.json")["ref_out"] == DIM7_OUT
    with pytest.raises(ValueError, match="positive definite"):
        XF.ldl_exact(json.load(open(os.path.join(C.GOLDEN, "lllgram_rankdef.json")))["G_in"])
    with pytest.raises(ValueError, match="symmetric"):
        XF.ldl_exact([[2, 1], [0, 2]])


# ---- 2. the model against the basis kernel's model, on the same mu / r ------------------------------------------------
def _same(b, K, bound=None, pruning=None):
    mu, r, e = _gso_of(b)
    want = BM.solve(b, mu, r, e, K, bound_sq=bound, pruning=pruning, row_expo=False)
    got = GM.solve(gram_of(b), mu, r, K, bound_sq=bound, pruning=pruning)
    for key in ("status", "found", "sol_coord", "norm", "nodes", "d_eff", "B0", "insertions"):
        assert got[key] == want[key], (key, K, bound)
    return got


@pytest.mark.parametrize("name", F.names())
def test_model_equals_the_basis_model_on_every_member(name):
    """The walk sees only mu and r, both evaluators decide on the same integers: found, sol_coord, norm and nodes are
    those of svp_best_model.solve, for K = 1, 5, 64, without a bound and at the third distinct norm."""
    b = F.basis(name)
    norms3, _ = F.norms_exact(name, 3)
    for bound in (None, norms3[2]):
        for K in (1, 5, 64):
            assert _same(b, K, bound)["status"] == 1


@pytest.mark.parametrize("name", F.PRUNED)
def test_model_equals_the_basis_model_under_pruning(name):
    b = F.basis(name)
    pr = F.pruning_of(name)
    for K in (1, 5, 64):
        _same(b, K, None, pr)
    tight = [1e-9] * len(b)  # a pruning that leaves nothing: found = 0, status 1
    o = _same(b, 5, None, tight)
    assert o["found"] == 0 and o["status"] == 1


# ---- 3. the model against the exact enumeration ------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.names())
def test_model_norms_are_the_exact_lists(name):
    b = F.basis(name)
    G = gram_of(b)
    mu, r = GM.gso_of_form(G)
    ex = F.exact(name)
    default, _ = XF.short_exact_form(G, ex["N0"], rows=ex["d_eff"], max_nodes=2 * F.NODE_CAP)
    norms3, third = F.norms_exact(name, 3)
    for bound, lst in ((None, default), (norms3[2], third)):
        want = [nv for nv, _ in lst]
        for K in (1, 5, 64):
            o = GM.solve(G, mu, r, K, bound_sq=bound)
            assert o["status"] == 1 and o["found"] == min(K, len(want)) and o["norm"][:o["found"]] == want[:K], (name, bound, K)
            for j in range(o["found"]):
                assert XF.sqnorm(G, o["sol_coord"][j]) == o["norm"][j]
            assert all(not any(o["sol_coord"][j]) and o["norm"][j] == 0 for j in range(o["found"], K))


def test_model_on_the_form_that_is_no_gram_matrix_of_an_integer_basis():
    f = _nobasis()
    G = f["G_out"]
    mu, r = GM.gso_of_form(G)
    rn = sorted(G[i][i] for i in range(7))
    for bound in (None, rn[2], rn[-1]):
        N = bound or min(rn[:XF.d_eff_exact_form(G)])
        rows = XF.d_eff_exact_form(G) if bound is None else None
        want = [nv for nv, _ in XF.short_exact_form(G, N, rows=rows)[0]]
        for K in (1, 5, 64):
            o = GM.solve(G, mu, r, K, bound_sq=bound)
            assert o["status"] == 1 and o["norm"][:o["found"]] == want[:K] and o["found"] == min(K, len(want))


# ---- 4. the 63-bit rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in F.names("scaled_root") if F.info(n)["log_s"] == 29])
def test_scaled_root_forms_near_2_61_are_exact(name):
    """Entries near 2^61, norms that are no doubles: status 1 and the exact norms."""
    b = F.basis(name)
    G = gram_of(b)
    assert max(abs(v) for row in G for v in row) > 2**58
    mu, r = GM.gso_of_form(G)
    o = GM.solve(G, mu, r, 5)
    ex = F.exact(name)
    want = [nv for nv, _ in XF.short_exact_form(G, ex["N0"], rows=ex["d_eff"], max_nodes=2 * F.NODE_CAP)[0]]
    assert o["status"] == 1 and o["norm"][:o["found"]] == want[:5] and o["found"] == min(5, len(want))


@pytest.mark.parametrize("name", sorted(BIG.CASES))
def test_partial_sums_beyond_63_bits_are_exact(name):
    """tests/svp_gram_cases.py: the kept vectors have a prefix of y_j = sum_i x_i g_ij of 2^63 and more (an
    overflow-checked 64-bit sum gives these forms up) and — except where K = 4 keeps only the shortest — a product
    x_j y_j of 2^63 and more, while x G x^T fits: status 1, the norms of the exact enumeration, every record exact."""
    G, bound, K = BIG.case(name)
    assert max(abs(v) for row in G for v in row) < 2**63
    mu, r = GM.gso_of_form(G)
    o = GM.solve(G, mu, r, K, bound_sq=bound)
    want = [nv for nv, _ in XF.short_exact_form(G, bound, max_nodes=F.NODE_CAP)[0]]
    assert o["status"] == 1 and o["found"] == min(K, len(want)) > 0 and o["norm"][:o["found"]] == want[:K]
    for x, nv in zip(o["sol_coord"][:o["found"]], o["norm"]):
        assert XF.sqnorm(G, x) == nv
    prefix, term = BIG.partial_bits(G, o["sol_coord"][:o["found"]])
    assert prefix >= 64, prefix  # (bit length 64: at least 2^63)
    assert term >= 64 or K == 4, term


def test_the_scaled_root_forms_do_not_need_the_128_bits():
    """What the scaled_root members do and do not show: entries near 2^61, but every prefix of every kept vector's
    sums fits 63 bits — they check exactness near the top of the range, the cases above check the wide sums."""
    for name in [n for n in F.names("scaled_root") if F.info(n)["log_s"] == 29]:
        G = gram_of(F.basis(name))
        mu, r = GM.gso_of_form(G)
        o = GM.solve(G, mu, r, 5)
        assert BIG.partial_bits(G, o["sol_coord"][:o["found"]])[0] <= 63


def test_the_evaluators_steps_on_adversarial_values():
    """form_norm's internal assertions (no 128-bit step leaves its range, the split sum is x G x^T) on entries and
    coefficients at the limits: |g_ij| = 2^63 - 1, |x_i| = 2^57 - 1, d = 64."""
    d = 64
    big = 2**63 - 1
    G = [[big if (i + j) % 2 == 0 else -big for j in range(d)] for i in range(d)]
    x = [float(2**57 - 2**5) * (1 if i % 2 == 0 else -1) for i in range(d)]
    assert GM.form_norm(G, x, d) == (False, 0)  # (far beyond 63 bits; the steps themselves held)
    assert GM.form_norm(G, [2.0**57] + [0.0] * 63, d) == (False, 0)
    assert GM.form_norm([[5, -7], [-7, 3]], [1.0, 1.0], 2) == (True, -1)  # indefinite: a negative value, not accepted
    assert GM.form_norm([[2**62, 0], [0, 2**62]], [1.0, 1.0], 2) == (False, 0)
    assert GM.form_norm([[2**62, -1], [-1, 2**62]], [1.0, 1.0], 2) == (True, 2**63 - 2)
    # the value beyond 2^64: the part above the low word is not zero
    assert GM.form_norm([[2**62, 0], [0, 2**62]], [3.0, 3.0], 2) == (False, 0)
    assert GM.form_norm([[2**62, 2**62 - 1], [2**62 - 1, 2**62]], [3.0, -3.0], 2) == (True, 18)  # prefixes of 3 2^62


def test_a_candidate_of_norm_2_63_is_status_minus_2():
    G = [[2**62, 0], [0, 2**62]]
    o = GM.solve(G, [[0.0, 0.0], [0.0, 0.0]], [2.0**62, 2.0**62], 4, bound_sq=2**63 - 1)
    assert o["status"] == -2 and o["found"] == 0 and o["nodes"] == 0 and not any(o["norm"])
    assert not any(any(x) for x in o["sol_coord"])
    # below it the same form answers
    o = GM.solve(G, [[0.0, 0.0], [0.0, 0.0]], [2.0**62, 2.0**62], 4)
    assert o["status"] == 1 and o["norm"] == [2**62, 2**62, 0, 0]
    # 2^56 [[64, 24], [24, 10]]: within 64 2^56 thirteen vectors, exact; under 2^63 - 1 a candidate of 2^63 and more
    s2 = 2**56
    G = [[64 * s2, 24 * s2], [24 * s2, 10 * s2]]
    mu, r = GM.gso_of_form(G)
    o = GM.solve(G, mu, r, 64, bound_sq=64 * s2)
    assert o["status"] == 1 and o["found"] == 13 and o["norm"][:13] == [nv for nv, _ in XF.short_exact_form(G, 64 * s2)[0]]
    assert BIG.partial_bits(G, o["sol_coord"][:13])[0] >= 64
    assert GM.solve(G, mu, r, 64, bound_sq=2**63 - 1)["status"] == -2


def test_forms_that_are_not_positive_definite_are_status_0():
    o = GM.solve([[2, 0], [0, 0]], [[0.0, 0.0], [0.0, 0.0]], [2.0, 0.0], 4)
    assert o["status"] == 0 and o["found"] == 0
    o = GM.solve([[2, 3], [3, 2]], [[0.0, 0.0], [1.5, 0.0]], [2.0, -2.5], 4)
    assert o["status"] == 0
    o = GM.solve([[2, 1], [1, 2]], [[0.0, 0.0], [float("nan"), 0.0]], [2.0, float("nan")], 4, update_status=0)
    assert o["status"] == 0
    # a row that is cut may be anything: only the rows walked are asked
    o = GM.solve([[2, 0], [0, 100]], [[0.0, 0.0], [0.0, 0.0]], [2.0, float("inf")], 4)
    assert o["status"] == 1 and o["d_eff"] == 1 and o["norm"] == [2, 0, 0, 0]


# ---- 5. the recorded runs of the reference ---------------------------------------------------------------------------
FIXTURES = sorted(glob.glob(os.path.join(C.GOLDEN, "svpgram_*.json")))


def test_the_fixture_set_is_complete():
    names = sorted(os.path.basename(p) for p in FIXTURES)
    assert names == sorted("svpgram_%s_k%d.json" % (s, k) for s in ("dim7", "dim4", "nobasis", "q24") for k in (8, 64))


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-5] for p in FIXTURES])
def test_reference_fixture(path):
    """The recorded coefficients have the recorded norms under the recorded (reduced) form; the sorted norms are the
    exact enumeration's first `found`; the first norm is that of the reference's held answer where there is one; the
    model returns the same norms."""
    f = json.load(open(path))
    G, K = f["G"], f["max_sols"]
    assert f["found"] == len(f["norm"]) == len(f["sol_coord"]) <= K and f["norm"] == sorted(f["norm"])
    for x, nv in zip(f["sol_coord"], f["norm"]):
        assert XF.sqnorm(G, x) == nv
    assert XF.sqnorm(G, f["sv_coord"]) == f["sv_norm"] == f["norm"][0]
    de = XF.d_eff_exact_form(G)
    B0 = min(G[i][i] for i in range(de))
    want = [nv for nv, _ in XF.short_exact_form(G, B0, rows=de, max_nodes=2 * F.NODE_CAP)[0]]
    assert f["norm"] == want[:f["found"]] and f["found"] == min(K, len(want))
    if "ref_out" in f:
        assert XF.sqnorm(f["G_in"], f["ref_out"]) == f["norm"][0]
    mu, r = GM.gso_of_form(G)
    o = GM.solve(G, mu, r, K)
    assert o["status"] == 1 and o["found"] == f["found"] and o["norm"][:o["found"]] == f["norm"]


# ---- 6. the wrappers' argument checks, the C ABI, the build -------------------------------------------------------------
def test_sqnorm_coordinates_and_argument_checks():
    from fplll_amd.gram import shortest_vectors_gram, sqnorm_coordinates
    assert sqnorm_coordinates(DIM7, DIM7_OUT) == 3
    assert sqnorm_coordinates([[2**62, 2**61], [2**61, 2**62]], [2**40, -2**40]) == 2**142 + 2**142 - 2 * 2**141
    with pytest.raises(ValueError, match="sqnorm_coordinates"):
        sqnorm_coordinates(DIM7, [1, 2])
    good = np.array(DIM7, dtype=np.int64)
    with pytest.raises(ValueError, match=r"\[d\]\[d\]"):
        shortest_vectors_gram(None, good[:3], 4)
    for K in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="max_sols"):
            shortest_vectors_gram(None, good, K)
    with pytest.raises(ValueError, match="route"):
        shortest_vectors_gram(None, good, 4, route="fastest")
    with pytest.raises(ValueError, match="pruning"):
        shortest_vectors_gram(None, good, 4, pruning=np.ones(4))
    with pytest.raises(ValueError, match="bound_sq"):
        shortest_vectors_gram(None, good, 4, bound_sq=-1)
    with pytest.raises(ValueError, match="bound_sq"):
        shortest_vectors_gram(None, good, 4, bound_sq=[1, 2])


def test_the_c_abi_has_the_solver(tmp_path):
    from fplll_amd import _lib
    lib = _lib.load()
    assert lib.fphip_abi_version() >= 9
    fn = _lib.bind_gram_shortest_vectors(lib)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    # no object: an error, nothing dereferenced
    assert fn(None, None, 0, 1, 4, None, 0, 0, None, 0, None, None, None, None, None) == -1
    hdr = os.path.join(C.ROOT, "include", "fplll_hip.h")
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n'
                   'int (*p)(fphip_gram *, fphip_ctx *, int, int, int, const int64_t *, int, int, const double *, int, int *,\n'
                   '         int64_t *, int64_t *, uint64_t *, int *) = fphip_gram_shortest_vectors;\n' % hdr)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_build_lists_the_kernel_with_the_flags_of_its_siblings():
    from fplll_amd import build
    assert "svp_gram.hip" in build.HIP_SOURCES and "svp_host.h" in build.HIP_HEADERS
    assert build.PER_FILE_FLAGS["svp_gram.hip"] == build.PER_FILE_FLAGS["svp_best.hip"] == build.PER_FILE_FLAGS["svp_wave.hip"]


LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]


def _kernels(src, tmp):
    """{mangled kernel name: (registers, scratch bytes per lane)} of one translation unit of the built library."""
    obj = os.path.join(C.ROOT, "fplll_amd", "lib", "obj", src + ".o")
    assert os.path.exists(obj), obj
    fat, co = os.path.join(tmp, src + ".fat"), os.path.join(tmp, src + ".co")
    subprocess.check_call([TOOLS[0], "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "unused.o")])
    subprocess.check_call([TOOLS[1], "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([TOOLS[2], "--notes", co]).decode()
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                     int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return out


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")
def test_kernel_has_no_scratch_and_the_registers_of_its_sibling(tmp_path):
    """svp_gram_kernel and nothing else is in the code object build() left behind, without scratch memory and with no
    more registers than svp_best_kernel<1> of the same build plus one allocation granule of 8: the same walk with the
    column loop removed."""
    from fplll_amd import build
    build.build_hip()
    seen = _kernels("svp_gram.hip", str(tmp_path))
    assert sorted(seen) == ["_ZN5fphip15svp_gram_kernelENS_9GramBatchENS_11SvpGramWaveE"], sorted(seen)
    (regs, scratch), = seen.values()
    best = _kernels("svp_best.hip", str(tmp_path))["_ZN5fphip15svp_best_kernelILi1EEEvNS_8GsoBatchENS_11SvpBestWaveE"]
    print("svp_gram_kernel: %d registers, %d bytes of scratch; svp_best_kernel<1>: %d registers" % (regs, scratch, best[0]))
    assert scratch == 0 and regs <= best[0] + 8, (regs, scratch, best)
