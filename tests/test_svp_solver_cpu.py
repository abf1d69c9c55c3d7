"""The shortest-vector solver (fplll_amd.svp.shortest_vector, fphip_shortest_vector, svp_wave.hip), the CPU half: the
kernel's model (tests/svp_model.py) against brute force and on lattices with known minima, the conditions of the
recorded fixtures (tests/golden/svpsolve_*.json, tests/golden/make_svp_solver_fixtures.sh), the argument checks of the
wrappers, the C ABI, and the kernel's names and scratch use read from the object build() left behind."""
import ctypes
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

import conftest as C
import list_helpers as H
import svp_model as M


def _solve(b, pruning=None):
    mu, r, e = M.gso_of(b)
    return M.solve(b, mu, r, e, pruning=pruning)


def _check_answer(b, o):
    """vec = sol_coord b, |vec|^2 = norm, sol_coord != 0: in Python integers."""
    v = [sum(int(o["sol_coord"][i]) * int(b[i][j]) for i in range(len(b))) for j in range(len(b[0]))]
    assert v == [int(t) for t in o["vec"]] and sum(t * t for t in v) == o["norm"] and any(o["sol_coord"])


# ---- 1. the model is a shortest-vector solver ------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,seed", [(2, 2, 0), (3, 5, 1), (4, 4, 2), (5, 7, 3), (6, 6, 4), (7, 7, 5), (8, 8, 6), (8, 11, 7)])
def test_model_against_brute_force(d, n, seed):
    """Seeded bases, LLL-reduced in rational arithmetic: the model's norm is the minimum over the coefficient box that
    the exact Gram matrix bounds."""
    rng = np.random.default_rng(seed)
    b = H.lll_exact(rng.integers(-40, 41, size=(d, n)).tolist())
    o = _solve(b)
    assert o["status"] == 1
    _check_answer(b, o)
    assert o["norm"] == M.brute_force_min(b)


def test_model_on_known_lattices():
    """Z^8 in a unimodular basis: norm 1, and the walk stops at the first vector of norm 1 (nothing non-zero is
    shorter); D4: 2; E8 (the basis spans 2 E8: 4 * 2); the Leech lattice (the reference's data file, scaled by
    sqrt 8: 8 * 4)."""
    for b, want in ((H.lll_exact(H.z8_basis()), 1), (H.d4_basis(), 2), (H.lll_exact(H.e8_basis()[0]), 8),
                    (H.leech_basis(), 32)):
        o = _solve(b)
        assert o["status"] == 1 and o["norm"] == want, (len(b), o["norm"])
        _check_answer(b, o)
    # a reduced basis that holds a vector of norm 1: the initial answer, no walk, no nodes
    b = [[1, 0, 0], [0, 3, 1], [0, 1, 4]]
    o = _solve(b)
    assert o["norm"] == 1 and o["nodes"] == 0 and o["sol_coord"] == [1, 0, 0]
    # Z^8's unimodular basis as it stands (not reduced): found by the walk
    o = _solve(H.z8_basis())
    assert o["norm"] == 1
    _check_answer(H.z8_basis(), o)


def test_model_keeps_the_first_of_tied_minima_and_a_basis_vector_when_nothing_is_shorter():
    """D4 has 24 minimal vectors, four of them rows of the basis: no candidate is STRICTLY shorter than the first row,
    so the answer is e_0 — after a walk that found nothing (its nodes are counted)."""
    o = _solve(H.d4_basis())
    assert o["sol_coord"] == [1, 0, 0, 0] and o["improvements"] == 0 and o["nodes"] > 0
    # the lowest index on ties of the initial answer: rows 1 and 2 tie below row 0
    b = [[3, 0, 0], [0, 2, 0], [0, 0, 2]]
    o = _solve(b)
    assert o["i0"] == 1 and o["sol_coord"] == [0, 1, 0] and o["norm"] == 4


def test_last_useful_index():
    """svpcvp.cpp:32-43: d_eff = 1 + the last i > 0 with r_ii <= 2 r_00 — the TRUE values, row exponents applied.  Rows
    at and above it keep coefficient 0, whatever they are."""
    assert M.last_useful_index([4.0, 9.0, 8.0, 8.5], [0] * 4) == 3
    assert M.last_useful_index([4.0, 9.0, 10.0], [0] * 3) == 1
    # stored values equal, exponents not: row 2 is 2^20 times longer (r 2^40 times), row 1 is not
    assert M.last_useful_index([1.0, 1.5, 1.0], [3, 3, 23]) == 2
    assert M.last_useful_index([1.0, 1.5, 1.0], [23, 3, 3]) == 3
    # the last two rows 2^20 times the others: their coefficients are 0 and the answer is that of the first rows
    top = [[10, 1, 0, 0, 1, 0], [0, 10, 1, 0, 0, 1], [1, 0, 10, 1, 0, 0], [0, 1, 0, 10, 1, 0]]  # r_ii about 100 each
    b = top + [[(1 << 20) * v for v in row] for row in ([1, -2, 0, 3, 5, 1], [2, 0, -1, 1, 1, 4])]
    o = _solve(b)
    assert o["d_eff"] == 4 and o["sol_coord"][4:] == [0, 0] and o["norm"] == _solve(top)["norm"]
    _check_answer(b, o)


def test_model_reports_a_row_beyond_63_bits():
    o = _solve([[1 << 62, 0], [0, 5]])
    assert o["status"] == -2 and o["norm"] == 0 and not any(o["sol_coord"]) and not any(o["vec"])


def test_model_takes_a_pruning_vector():
    """Linear pruning cuts the tree; the bound of level k is pruning[k] * radius."""
    b = json.load(open(os.path.join(C.GOLDEN, "svpsolve_q24_s1.json")))["basis"]
    full = _solve(b)
    pr = [0.5 + 0.5 * (k + 1) / 24 for k in range(24)]  # from 0.52 at the leaves up to 1 at the top level
    pruned = _solve(b, pruning=pr)
    assert pruned["status"] == 1 and pruned["nodes"] < full["nodes"] and pruned["norm"] >= full["norm"]
    _check_answer(b, pruned)


# ---- 2. the fixtures --------------------------------------------------------------------------------------------------
FIXTURES = sorted(glob.glob(os.path.join(C.GOLDEN, "svpsolve_q*.json")))


def test_fixture_set():
    """q-ary at d = 24, 32, 40, two seeds each; the reference's example pair; the rank-defect matrix."""
    dims = sorted(json.load(open(f))["d"] for f in FIXTURES)
    assert dims == [24, 24, 32, 32, 40, 40]
    for name in ("example_svp_in.txt", "example_svp_out.txt", "svp_rank_defect.json"):
        assert os.path.exists(os.path.join(C.GOLDEN, name))
    b = M_example_in()
    assert b.shape == (20, 21) and len(M_example_out()) == 21


def M_example_in():
    txt = open(os.path.join(C.GOLDEN, "example_svp_in.txt")).read().replace("[", " ").replace("]", " ")
    return np.array([int(t) for t in txt.split()], dtype=np.int64).reshape(20, 21)


def M_example_out():
    txt = open(os.path.join(C.GOLDEN, "example_svp_out.txt")).read().replace("[", " ").replace("]", " ")
    return [int(t) for t in txt.split()]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-5] for f in FIXTURES])
def test_fixture_conditions(path):
    """Each recorded instance: both methods succeeded (RED_SUCCESS is 0 in the reference), FAST norm == PROVED norm,
    the recorded norms are those of the recorded sol_coord, and norm <= the smallest row norm."""
    fx = json.load(open(path))
    b = fx["basis"]
    assert len(b) == fx["d"] and all(len(r) == fx["n"] for r in b)
    for m in ("fast", "proved"):
        assert fx[m]["status"] == 0
        v = [sum(int(fx[m]["sol_coord"][i]) * int(b[i][j]) for i in range(fx["d"])) for j in range(fx["n"])]
        assert sum(t * t for t in v) == fx[m]["norm"] > 0
        assert fx[m]["ref_ms"] > 0
    assert fx["fast"]["norm"] == fx["proved"]["norm"]
    assert fx["fast"]["norm"] <= min(sum(int(t) ** 2 for t in r) for r in b)
    assert max(abs(int(t)) for r in b for t in r) < 2**11


@pytest.mark.parametrize("path", [f for f in FIXTURES if json.load(open(f))["d"] <= 32],
                         ids=lambda f: os.path.basename(f)[:-5])
def test_model_finds_the_references_norm(path):
    """d = 24 and 32 (the d = 40 trees take the model a minute): the model, fed with mu and r rounded from the exact
    rationals, ends on the reference's norm."""
    fx = json.load(open(path))
    o = _solve(fx["basis"])
    assert o["status"] == 1 and o["norm"] == fx["fast"]["norm"]
    _check_answer(fx["basis"], o)


def test_example_pair_and_rank_defect():
    """example_svp_out is a shortest vector of example_svp_in's lattice (the model on the exactly reduced basis finds
    its norm); the rank-defect matrix reduces and solves."""
    want = sum(t * t for t in M_example_out())
    b = H.lll_exact(M_example_in().tolist())
    o = _solve(b)
    assert o["status"] == 1 and o["norm"] == want
    rd = json.load(open(os.path.join(C.GOLDEN, "svp_rank_defect.json")))["basis"]
    b = H.lll_exact(rd)
    o = _solve(b)
    assert o["status"] == 1 and o["norm"] == M.brute_force_min(b)
    _check_answer(b, o)


# ---- 3. the wrappers and the C ABI -----------------------------------------------------------------------------------
def test_wrappers_check_their_arguments():
    """Every check comes before the context is touched (ctx = None here)."""
    from fplll_amd.svp import shortest_vector, shortest_vector_batch
    good = np.eye(3, 4, dtype=np.int64)
    with pytest.raises(ValueError, match=r"\[d\]\[n\]"):
        shortest_vector(None, np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match=r"\[d\]\[n\]"):
        shortest_vector(None, np.zeros((5, 3), dtype=np.int64))  # more rows than columns
    with pytest.raises(ValueError, match=r"\[B\]\[d\]\[n\]"):
        shortest_vector_batch(None, good)
    with pytest.raises(ValueError, match=r"\[B\]\[d\]\[n\]"):
        shortest_vector_batch(None, np.zeros((0, 3, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="route"):
        shortest_vector(None, good, route="fastest")
    with pytest.raises(ValueError, match="pruning"):
        shortest_vector(None, good, pruning=np.ones(4))


def test_the_c_abi_has_the_solver(tmp_path):
    from fplll_amd import _lib
    lib = _lib.load()
    assert lib.fphip_abi_version() >= 6
    fn = _lib.bind_shortest_vector(lib)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert (_lib.SVPM_FAST, _lib.SVPM_PROVED, _lib.SVP_OVERRIDE_BND, _lib.SVP_DUAL) == (0, 2, 2, 4)
    # no object: an error, nothing dereferenced
    assert fn(None, None, 0, 1, 0, 0, None, 0, None, None, None, None, None) == -1
    hdr = os.path.join(C.ROOT, "include", "fplll_hip.h")
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n'
                   'int (*p)(fphip_gso *, fphip_ctx *, int, int, int, int, const double *, int, int64_t *, int64_t *,\n'
                   '         int64_t *, uint64_t *, int *) = fphip_shortest_vector;\n'
                   'int v[] = {FPHIP_SVPM_FAST, FPHIP_SVPM_PROVED, FPHIP_SVP_OVERRIDE_BND, FPHIP_SVP_DUAL,\n'
                   '           FPHIP_SVP_ROUTE_AUTO, FPHIP_SVP_ROUTE_WAVE, FPHIP_SVP_ROUTE_ENUM};\n' % hdr)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_build_lists_the_kernel_with_the_flag_of_its_twin():
    from fplll_amd import build
    assert "svp_wave.hip" in build.HIP_SOURCES
    assert build.PER_FILE_FLAGS["svp_wave.hip"] == build.PER_FILE_FLAGS["bkz_kernel.hip"]
    assert "-structurizecfg-skip-uniform-regions=1" in build.PER_FILE_FLAGS["svp_wave.hip"]


LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")
def test_walk_kernels_of_all_four_widths_compile_without_scratch(tmp_path):
    """svp_wave_kernel<1..4> are in the code object build() left behind, each without scratch memory and within the
    128 registers that five waves per SIMD allow (DESIGN section 3f records the figures as built)."""
    from fplll_amd import build
    build.build_hip()
    obj = os.path.join(C.ROOT, "fplll_amd", "lib", "obj", "svp_wave.hip.o")
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
    want = ["_ZN5fphip15svp_wave_kernelILi%dEEEvNS_8GsoBatchENS_7SvpWaveE" % nq for nq in (1, 2, 3, 4)]
    assert sorted(seen) == want, sorted(seen)
    for k, (regs, scratch) in seen.items():
        assert scratch == 0 and regs <= 128, (k, regs, scratch)
