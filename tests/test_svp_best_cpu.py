"""The N-shortest-vectors solver (fplll_amd.svp.shortest_vectors, fphip_shortest_vectors, svp_best.hip), the CPU half:
the kernel's model (tests/svp_best_model.py) against the exact rational enumeration (tests/exact_lattice.py) on every
member of tests/solver_families.py and on lattices with known shells, the generalised row cut, three deliberate
mistakes in the model that these checks must catch, the recorded N-best runs of the reference
(tests/golden/svpbest_*.json), the wrappers' argument checks, the C ABI, and the kernel's names, registers and scratch
use read from the object build() left behind."""
import ctypes
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

import conftest as C
import exact_lattice as X
import list_helpers as H
import solver_families as F
import svp_best_model as BM
import svp_model as M

_gso = {}


def _gso_of(b):
    key = tuple(tuple(r) for r in b)
    if key not in _gso:
        _gso[key] = M.gso_of(b)
    return _gso[key]


def _solve(b, K, bound=None, **kw):
    mu, r, e = _gso_of(b)
    return BM.solve(b, mu, r, e, K, bound_sq=bound, **kw)


def _valid(b, o):
    """found <= K records, sorted by norm, each with vec = sol_coord b and |vec|^2 = norm in Python integers, non-zero,
    distinct modulo +-; the entries beyond found are zero."""
    K, f = len(o["norm"]), o["found"]
    seen = set()
    for j in range(K):
        x, v, nv = o["sol_coord"][j], o["vec"][j], o["norm"][j]
        if j >= f:
            assert not any(x) and not any(v) and nv == 0
            continue
        assert X.vector_of(b, x) == [int(t) for t in v] and sum(int(t) ** 2 for t in v) == nv > 0
        assert j == 0 or o["norm"][j - 1] <= nv
        key = tuple(int(t) for t in x)
        assert key not in seen and tuple(-t for t in key) not in seen
        seen.add(key)


def _q24():
    return json.load(open(os.path.join(C.GOLDEN, "svpsolve_q24_s1.json")))["basis"]


# ---- 1. the model against the exact enumeration, every member --------------------------------------------------------
@pytest.mark.parametrize("name", F.names())
def test_model_against_the_exact_list_on_every_member(name):
    """At the default bound (the rows below last_useful_index) and at the third distinct norm of the lattice (all rows:
    a caller's bound), for K = 1, 5, 64: the model's norms are the first K of the exact list."""
    b = F.basis(name)
    ex = F.exact(name)
    default, _ = X.short_exact(b, ex["N0"], rows=ex["d_eff"], max_nodes=2 * F.NODE_CAP)
    norms3, third = F.norms_exact(name, 3)
    for bound, lst in ((None, default), (norms3[2], third)):
        want = [nv for nv, _ in lst]
        for K in (1, 5, 64):
            o = _solve(b, K, bound)
            assert o["status"] == 1
            if bound is None:
                assert o["d_eff"] == ex["d_eff"] and o["B0"] == ex["N0"]
            assert o["norm"][:o["found"]] == want[:K] and o["found"] == min(K, len(want)), (name, bound, K)
            _valid(b, o)


@pytest.mark.parametrize("name", F.names())
def test_one_vector_is_the_shortest_vector_models_norm(name):
    """K = 1 at the default bound ends on svp_model.solve's norm (the inclusive start finds the row that the other
    solver is seeded with)."""
    b = F.basis(name)
    mu, r, e = _gso_of(b)
    o = _solve(b, 1)
    assert o["found"] == 1 and o["norm"][0] == M.solve(b, mu, r, e)["norm"]


# ---- 2. known shells --------------------------------------------------------------------------------------------------
def _known_counts(solve):
    z8 = H.lll_exact(H.z8_basis())
    o = solve(z8, 8)
    assert o["found"] == 8 and o["norm"] == [1] * 8
    # (it stops: a full table with worst = 1 ends the walk — a table of three ends it before the fourth is met)
    o3 = solve(z8, 3)
    assert o3["norm"] == [1] * 3 and o3["insertions"] == 3 and o3["nodes"] < o["nodes"]
    assert solve(z8, 16)["found"] == 8
    o = solve(z8, 64, 2)  # 8 of norm 1 and C(8,2) * 2 = 56 of norm 2, one of each pair: the table fills on the last
    assert o["found"] == 64 and o["norm"] == [1] * 8 + [2] * 56 and o["insertions"] == 64
    _valid(z8, o)
    d4 = H.d4_basis()
    assert solve(d4, 12)["norm"] == [2] * 12
    o5 = solve(d4, 5)
    assert o5["found"] == 5 and o5["norm"] == [2] * 5
    for K in (24, 64):
        o = solve(d4, K, 4)
        assert o["found"] == 24 and o["norm"][:24] == [2] * 12 + [4] * 12
        _valid(d4, o)
    e8 = H.lll_exact(H.e8_basis()[0])
    o = solve(e8, 64)  # 120 pairs of norm 8: ties at the cut, norms and validity only
    assert o["found"] == 64 and o["norm"] == [8] * 64
    _valid(e8, o)
    return o5


def test_known_counts():
    _known_counts(_solve)
    leech = H.leech_basis()
    o = _solve(leech, 64)
    assert o["found"] == 64 and o["norm"] == [32] * 64
    _valid(leech, o)


def _discovery_order(solve):
    """Ties stay in discovery order: the five D4 vectors a table of five keeps are the first five of the twelve that
    a table of twelve keeps, in the same order; and in Z^8 at bound 2 the records of each norm come in the order of
    the walk whatever K cuts off."""
    d4 = H.d4_basis()
    assert solve(d4, 5)["sol_coord"] == solve(d4, 12)["sol_coord"][:5]
    z8 = H.lll_exact(H.z8_basis())
    assert solve(z8, 8, 2)["sol_coord"] == solve(z8, 64, 2)["sol_coord"][:8]


def test_ties_stay_in_discovery_order():
    _discovery_order(_solve)


# ---- 3. the rows cut ---------------------------------------------------------------------------------------------------
def _row_cut(solve):
    b = [[3, 0], [1, 5]]  # r = 9, 25: 25 > 2 r_00, and eight of the nine vectors within 100 use row 1
    o = solve(b, 64, 100)
    assert o["norm"][:o["found"]] == [9, 26, 29, 36, 41, 50, 74, 81, 89]
    assert [nv for nv, _ in X.short_exact(b, 100)[0]] == [9, 26, 29, 36, 41, 50, 74, 81, 89]
    b = F.basis("cut_cut")  # the last row has r = 577 = 2 r_00 + 1: cut by default, kept under the bound 577
    o = solve(b, 64, 577)
    assert o["found"] == 17 and o["d_eff"] == 5
    assert sum(1 for x in o["sol_coord"][:17] if x[4] != 0) == 1
    assert o["norm"][:17] == [nv for nv, _ in X.short_exact(b, 577)[0]]
    _valid(b, o)


def test_rows_cut_under_a_callers_bound():
    _row_cut(_solve)
    # the default bound: bit for bit the other solver's d_eff
    for name in F.names("cut_rows"):
        b = F.basis(name)
        mu, r, e = _gso_of(b)
        assert _solve(b, 3)["d_eff"] == M.solve(b, mu, r, e)["d_eff"] == F.exact(name)["d_eff"]


def test_one_row():
    """d = 1 (and d_eff = 1): the answers are the multiples of b_0."""
    b = [[7, 2, 1, 0]]
    o = _solve(b, 5, 54 * 9)
    assert o["found"] == 3 and o["norm"] == [54, 216, 486, 0, 0] and o["sol_coord"][:3] == [[1], [2], [3]]
    _valid(b, o)
    o = _solve(b, 2, 54 * 100)
    assert o["found"] == 2 and o["norm"] == [54, 216]
    o = _solve(b, 4)
    assert o["found"] == 1 and o["norm"][0] == 54
    b = [[2, 0, 0], [0, 9, 0], [0, 0, 9]]  # d_eff = 1 of 3 at the default bound
    o = _solve(b, 4)
    assert o["d_eff"] == 1 and o["found"] == 1 and o["sol_coord"][0] == [1, 0, 0]
    o = _solve(b, 4, 16)  # bound 16 < 81: still one row, the multiples 1 and 2
    assert o["d_eff"] == 1 and o["norm"] == [4, 16, 0, 0]


# ---- 4. the partial fill and the shrink on the recorded q-ary basis --------------------------------------------------
_q24_exact = {}


def _q24_list(bound):
    if bound not in _q24_exact:
        _q24_exact[bound] = [nv for nv, _ in X.short_exact(_q24(), bound)[0]]
    return _q24_exact[bound]


def _partial_and_shrink(solve):
    b = _q24()
    o = solve(b, 64, 3181)  # 26 vectors within the bound: the table never fills, the radius never shrinks
    assert o["found"] == 26 and o["norm"][:26] == _q24_list(3181) and len(_q24_list(3181)) == 26
    _valid(b, o)
    want = _q24_list(3817)
    assert len(want) == 233 and want[63] == 3429 and want[64] > 3429  # no tie at the cut
    o = solve(b, 64, 3817)
    assert o["found"] == 64 and o["norm"] == want[:64]
    _valid(b, o)
    return o


Q24_NODES_3817 = 29510  # the model's count on gso_of's doubles with the radius at worst - 1 = 3428 (this module pins it)


def test_partial_fill_and_shrink():
    o = _partial_and_shrink(_solve)
    assert o["nodes"] == Q24_NODES_3817
    for K in (1, 5):
        assert _solve(_q24(), K, 3817)["norm"] == _q24_list(3817)[:K]


def test_pruning_can_leave_nothing():
    """With pruning found may be 0 while status stays 1 (the reference's RED_ENUM_FAILURE case)."""
    o = _solve(H.d4_basis(), 4, pruning=[0.01] * 4)
    assert o["status"] == 1 and o["found"] == 0 and o["norm"] == [0] * 4


def test_model_reports_a_row_beyond_63_bits():
    o = _solve([[1 << 62, 0], [0, 5]], 3)
    assert o["status"] == -2 and o["found"] == 0 and o["norm"] == [0] * 3 and not any(any(x) for x in o["sol_coord"])


# ---- 5. three mistakes these checks catch ------------------------------------------------------------------------------
def _mutant(kind):
    return lambda b, K, bound=None, **kw: _solve(b, K, bound, mutate=kind, **kw)


def test_mutation_radius_at_worst():
    """The radius of a full table at `worst` instead of `worst - 1`: the answer is the same (the accept rule is the
    integers'), the walk is larger — caught by the node count of the shrink case."""
    o = _partial_and_shrink(_mutant("radius_at_worst"))
    assert o["nodes"] > Q24_NODES_3817


def test_mutation_reference_row_cut():
    """The 2 r_00 rule under a caller's bound drops every vector that uses row 1 of [[3, 0], [1, 5]]: three left."""
    m = _mutant("reference_row_cut")
    assert m([[3, 0], [1, 5]], 64, 100)["norm"][:3] == [9, 36, 81] and m([[3, 0], [1, 5]], 64, 100)["found"] == 3
    with pytest.raises(AssertionError):
        _row_cut(m)


def test_mutation_ties_in_front():
    with pytest.raises(AssertionError):
        _discovery_order(_mutant("ties_in_front"))


# ---- 6. the reference's own N-best -------------------------------------------------------------------------------------
REF_FIXTURES = sorted(glob.glob(os.path.join(C.GOLDEN, "svpbest_*.json")))


def test_reference_fixture_set():
    got = sorted((json.load(open(f))["source"], json.load(open(f))["bound_sq"], json.load(open(f))["max_sols"]) for f in REF_FIXTURES)
    assert got == sorted((s, bd, K) for s, bd in (("svpsolve_q24_s1", 3181), ("svpsolve_q24_s1", 3817), ("svpsolve_q32_s2", 5620))
                         for K in (8, 64))


@pytest.mark.parametrize("path", REF_FIXTURES, ids=lambda f: os.path.basename(f)[:-5])
def test_reference_n_best_norms_are_the_models(path):
    """The recorded norms are those of the recorded coefficients, and equal the model's (the reference's evaluator
    decides in floating point: where it keeps another vector at a tie only the norm lists are compared)."""
    fx = json.load(open(path))
    b = json.load(open(os.path.join(C.GOLDEN, fx["source"] + ".json")))["basis"]
    assert fx["basis"] == b
    assert len(fx["sol_coord"]) == len(fx["norm"]) == fx["found"] <= fx["max_sols"]
    for x, nv in zip(fx["sol_coord"], fx["norm"]):
        assert sum(t * t for t in X.vector_of(b, x)) == nv
    assert fx["norm"] == sorted(fx["norm"])
    o = _solve(b, fx["max_sols"], fx["bound_sq"])
    assert o["norm"][:o["found"]] == fx["norm"]


# ---- 7. the wrappers and the C ABI -----------------------------------------------------------------------------------
def test_wrappers_check_their_arguments():
    """Every check comes before the context is touched (ctx = None here)."""
    from fplll_amd.svp import shortest_vectors, shortest_vectors_batch
    import fplll_amd
    assert fplll_amd.shortest_vectors is shortest_vectors and fplll_amd.shortest_vectors_batch is shortest_vectors_batch
    good = np.eye(3, 4, dtype=np.int64)
    with pytest.raises(ValueError, match=r"\[d\]\[n\]"):
        shortest_vectors(None, np.zeros(5, dtype=np.int64), 4)
    with pytest.raises(ValueError, match=r"\[d\]\[n\]"):
        shortest_vectors(None, np.zeros((5, 3), dtype=np.int64), 4)
    with pytest.raises(ValueError, match=r"\[B\]\[d\]\[n\]"):
        shortest_vectors_batch(None, good, 4)
    for K in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="short_vectors"):
            shortest_vectors(None, good, K)
    with pytest.raises(ValueError, match="route"):
        shortest_vectors(None, good, 4, route="fastest")
    with pytest.raises(ValueError, match="pruning"):
        shortest_vectors(None, good, 4, pruning=np.ones(4))
    with pytest.raises(ValueError, match="bound_sq"):
        shortest_vectors(None, good, 4, bound_sq=-1)
    with pytest.raises(ValueError, match="bound_sq"):
        shortest_vectors(None, good, 4, bound_sq=[1, 2])
    with pytest.raises(ValueError, match="bound_sq"):
        shortest_vectors_batch(None, good[None], 4, bound_sq=[1, 2])
    with pytest.raises(ValueError, match="bound_sq"):
        shortest_vectors_batch(None, good[None], 4, bound_sq=2.5)


def test_the_c_abi_has_the_solver(tmp_path):
    from fplll_amd import _lib
    lib = _lib.load()
    assert lib.fphip_abi_version() >= 8
    fn = _lib.bind_shortest_vectors(lib)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
    # no object: an error, nothing dereferenced
    assert fn(None, None, 0, 1, 4, None, 0, 0, None, 0, None, None, None, None, None, None) == -1
    hdr = os.path.join(C.ROOT, "include", "fplll_hip.h")
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n'
                   'int (*p)(fphip_gso *, fphip_ctx *, int, int, int, const int64_t *, int, int, const double *, int, int *,\n'
                   '         int64_t *, int64_t *, int64_t *, uint64_t *, int *) = fphip_shortest_vectors;\n' % hdr)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_build_lists_the_kernel_with_the_flags_of_its_twin():
    from fplll_amd import build
    assert "svp_best.hip" in build.HIP_SOURCES
    assert build.PER_FILE_FLAGS["svp_best.hip"] == build.PER_FILE_FLAGS["svp_wave.hip"]


LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")
def test_kernels_of_all_four_widths_compile_without_scratch(tmp_path):
    """svp_best_kernel<1..4> and nothing else are in the code object build() left behind, each without scratch memory
    and within svp_wave_kernel's budget of 128 registers: the table costs neither."""
    from fplll_amd import build
    build.build_hip()
    obj = os.path.join(C.ROOT, "fplll_amd", "lib", "obj", "svp_best.hip.o")
    assert os.path.exists(obj), obj
    fat, co = str(tmp_path / "svp.fat"), str(tmp_path / "svp.co")
    subprocess.check_call([TOOLS[0], "--dump-section", ".hip_fatbin=" + fat, obj, str(tmp_path / "unused.o")])
    subprocess.check_call([TOOLS[1], "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([TOOLS[2], "--notes", co]).decode()
    seen = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        seen[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                      int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    want = ["_ZN5fphip15svp_best_kernelILi%dEEEvNS_8GsoBatchENS_11SvpBestWaveE" % nq for nq in (1, 2, 3, 4)]
    assert sorted(seen) == want, sorted(seen)
    for k, (regs, scratch) in seen.items():
        assert scratch == 0 and regs <= 128, (k, regs, scratch)
