"""The closest-vector wave route (fphip_closest_vector_ex, cvp_wave.hip), the CPU half: the kernel's model
(tests/cvp_wave_model.py) against the exact rational tie blocks (tests/exact_cvp.py), against the exact integer
closest points of the seeded families (tests/exact_lattice.py, tests/solver_families.py) and against the reference's
recorded answers (tests/golden/cvpsolve_*.json); the node budget; three deliberate mistakes of the model, each noticed
by a case here; the identity behind the reduced target; the C ABI, the build and the wrappers' argument checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import conftest as C
import cvp_solver_cases as S
import cvp_wave_model as M
import exact_cvp as E
import exact_lattice as X
import solver_families as F

BLOCKS = ["dy12t", "dy20t", "q2t", "z8t"]  # (pr28t is pruned: the wave route has no pruning)
FAMILY = F.names("scaled_root", "knapsack", "wide") + ["steep_63", "steep_64"]
FIXTURES = dict(S.solver_fixtures())
MISTAKES = ["half_tree", "strict", "ties_even"]
_state = {}


def _gso(b):
    return S.true_values(*S.gso_double(np.array(b, dtype=object)), None)


def _targets(name):
    return np.array([t for _, t in F.targets(name)], dtype=object)


def _closest(name, k):
    key = ("closest", name, k)  # (shared with test_solvers_exact_gpu.py: computed once per process)
    if key not in F._exact:
        F._exact[key] = X.closest_exact(F.basis(name), F.targets(name)[k][1], max_nodes=F.NODE_CAP)
    return F._exact[key]


# ---- the walk against the exact tie blocks ---------------------------------------------------------------------------
def _recorded_walk(name, **mistake):
    mut, rdiag, pruning, R, target = E.CVP_BLOCKS[name]()
    assert pruning is None
    rec = []
    w = M.walk(np.asarray(mut).T, rdiag, target, R, lambda x, nd, radius: rec.append((nd, tuple(x))), **mistake)
    return sorted(rec), w


def _walk_equals_exact(name, **mistake):
    rec, w = _recorded_walk(name, **mistake)
    _, cands, stats = E.exact_of(name)
    return rec == cands and w["plain"] == stats["plain"] and w["status"] == 1 and w["nodes"] == sum(stats["plain"])


@pytest.mark.parametrize("name", BLOCKS)
def test_walk_visits_the_exact_set_of_the_tie_blocks(name):
    """A recording on_leaf at a fixed radius: the candidates (distance 0 and distances AT the bound included) and the
    plain per-level counts of the exact rational reference.  Every centre of q2t is an integer or a half-integer, every
    centre of z8t is 1/2."""
    assert _walk_equals_exact(name)


def test_the_tie_blocks_hold_what_they_are_for():
    stats = [E.exact_of(name)[2] for name in BLOCKS]
    assert sum(s["at_bound"] for s in stats) > 0 and sum(s["half_centres"] for s in stats) > 0


# ---- solve: the seeded families, the recorded fixtures ---------------------------------------------------------------
def _family_answer(name, **mistake):
    key = (name,) + tuple(sorted(mistake))
    if key not in _state:
        b = F.basis(name)
        mu, rd = _gso(b)
        _state[key] = M.solve(b, mu, rd, _targets(name), **mistake)
    return _state[key]


def _family_is_exact(name, **mistake):
    o, b = _family_answer(name, **mistake), F.basis(name)
    for k, (kind, t) in enumerate(F.targets(name)):
        d0, xs, _ = _closest(name, k)
        sol = tuple(int(v) for v in o["sol_coord"][k])
        if not (o["status"][k] == 1 and o["norm"][k] == d0 and sol in set(xs)
                and sum(v * v for v in X.vector_of(b, sol, t)) == d0):
            return False
    return True


@pytest.mark.parametrize("name", FAMILY)
def test_solve_finds_exact_closest_points_on_the_families(name):
    """Near, far (coefficients around 2^30) and halfway targets of every member: norm is closest_exact's distance, the
    answer one of its closest points (where they tie, any), norm the distance of the answer in Python integers."""
    assert _family_is_exact(name), name


def _fixture_answer(name, **mistake):
    fx = FIXTURES[name]
    b = S.basis_of(fx)
    mu, rd = _gso(b)
    return M.solve(b, mu, rd, S.targets_of(fx), **mistake)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_solve_returns_the_recorded_sol_coord(name):
    """The reference's closest_vector answers (lattice-point and far targets included).  The near:10 target of q36 is
    a tree of 1.2 million nodes: three seconds of Python, the one slow case."""
    fx = FIXTURES[name]
    o = _fixture_answer(name)
    assert o["sol_coord"] == [[int(v) for v in t["sol_coord"]] for t in fx["targets"]]
    assert o["status"] == [1] * len(fx["targets"])
    for k, t in enumerate(fx["targets"]):
        if t["kind"] == "lattice":  # not walked: the descent, distance 0
            assert o["nodes"][k] == 0 and o["norm"][k] == 0 and o["found"][k] == 0 and o["dist"][k] == 0.0
        else:
            assert o["found"][k] == 1 and o["nodes"][k] >= len(fx["basis"])
    C.note(lambda: ("%s: nodes per target %s" % (name, o["nodes"]),))


# ---- ties: the first candidate wins ----------------------------------------------------------------------------------
def _tie_case(**mistake):
    b = 2 * np.eye(8, dtype=np.int64)
    mu, rd = _gso(b)
    return M.solve(b, mu, rd, np.ones((1, 8), dtype=np.int64), **mistake)


def _tie_case_is_right(**mistake):
    """2 I_8 around (1, .., 1): 256 closest points at distance 8.  The first candidate wins and later ones only with a
    strictly smaller distance, so the answer is the first leaf of the walk — the rounding descent's point, which the
    preparation (not the walk) names: every centre is 1/2 and rounds away from zero, to 1.  All 256 tied leaves are
    candidates: the radius stays at the first one's distance, 255 + 255 nodes in all."""
    o = _tie_case(**mistake)
    return o["sol_coord"] == [[1] * 8] and o["norm"] == [8] and o["nodes"] == [510] and o["status"] == [1]


def test_a_256_way_tie_keeps_the_first_candidate():
    assert _tie_case_is_right()


def test_edges_two_rows_and_one_row():
    b = np.array([[3, 1], [1, 4]], dtype=np.int64)
    mu, rd = _gso(b)
    o = M.solve(b, mu, rd, np.array([[7, 9], [4, 5]], dtype=np.int64))
    for k, t in enumerate(([7, 9], [4, 5])):
        d0, xs, _ = X.closest_exact(b.tolist(), t)
        assert o["norm"][k] == d0 and tuple(o["sol_coord"][k]) in set(xs)
    assert o["nodes"][0] >= 2 and o["nodes"][1] == 0  # (4, 5) = b_0 + b_1: a lattice point is not walked
    b1 = np.array([[5, 0, 0]], dtype=np.int64)  # one row: never walked, the descent is the answer
    mu, rd = _gso(b1)
    o = M.solve(b1, mu, rd, np.array([[12, 1, 0], [13, 0, 0]], dtype=np.int64))
    assert o["sol_coord"] == [[2], [3]] and o["norm"] == [5, 4] and o["nodes"] == [0, 0] and o["found"] == [0, 0]


# ---- the budget ------------------------------------------------------------------------------------------------------
def test_budget_ends_the_walk_with_the_best_so_far():
    """knap_d20_b30's first near target is a tree of about 2 000 nodes: under max_nodes = 500 the walk ends at the
    first pass of the STEP loop that finds the count at or above 500, status 2, with a lattice point no closer than
    the closest; without a budget the answer is exact."""
    name = "knap_d20_b30"
    b, t = F.basis(name), F.targets(name)[0][1]
    mu, rd = _gso(b)
    tg = np.array([t], dtype=object)
    full = M.solve(b, mu, rd, tg)
    cut = M.solve(b, mu, rd, tg, max_nodes=500)
    d0, xs, _ = _closest(name, 0)
    assert full["status"] == [1] and 1500 <= full["nodes"][0] <= 3000
    assert full["norm"] == [d0] and tuple(full["sol_coord"][0]) in set(xs)
    assert cut["status"] == [M.NODE_LIMIT] and 500 <= cut["nodes"][0] < 500 + len(b) and cut["found"] == [1]
    got = sum(v * v for v in X.vector_of(b, cut["sol_coord"][0], t))
    assert got == cut["norm"][0] >= d0
    C.note(lambda: ("budget: %d nodes without, %d with; norm %d / %d" % (full["nodes"][0], cut["nodes"][0], d0, got),))


# ---- three deliberate mistakes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", MISTAKES)
def test_a_deliberate_mistake_is_noticed(mistake):
    """The shortest-vector walk's half-tree step at partial distance 0 and `<` for `<=` at the bound change the visited
    set of the tie blocks; ties rounded to even visit the same set in another order, which the first-candidate rule
    shows on the 256-way tie (the first leaf is no longer the rounding descent's point)."""
    noticed = [name for name in BLOCKS if not _walk_equals_exact(name, **{mistake: True})]
    if not _tie_case_is_right(**{mistake: True}):
        noticed.append("tie")
    C.note(lambda: ("mistake %s: noticed by %s" % (mistake, noticed),))
    assert noticed, mistake


# ---- the reduced target ----------------------------------------------------------------------------------------------
def _gscoords(b, mu, rd, t):
    """get_gscoords in the preparation's operation order (cvp_prepare.hip), one target."""
    bf = np.asarray(b, dtype=np.int64).astype(np.float64)
    d, n = bf.shape
    v = np.array([float(u) for u in t])
    c = np.zeros(d)
    for i in range(d):
        acc = 0.0
        for j in range(n):
            acc = acc + v[j] * bf[i, j]
        for j in range(i):
            acc = acc - mu[i, j] * c[j]
        c[i] = acc
    return np.array([c[i] / rd[i] for i in range(d)])


@pytest.mark.parametrize("name,kind", [("root_e8_s20_full_0", "half"), ("root_e8_s20_full_0", "far"), ("knap_d16_b40", "far")])
def test_target_coord_belongs_to_target_minus_coef_b(name, kind):
    """t_red = target - sum coef_i b_i is the vector whose Gram-Schmidt coordinates are target_coord — also at the
    preparation's `undo` exit (the halfway target: three passes), where coef and the running target are those of the
    last completed subtraction."""
    b = F.basis(name)
    mu, rd = _gso(b)
    k = [kd for kd, _ in F.targets(name)].index(kind)
    t = F.targets(name)[k][1]
    P = S.prepare(b, mu, rd, np.array([t], dtype=object))
    assert P["status"][0] == 1 and P["passes"][0] >= 2 and np.any(P["coef"][0] != 0)
    t_red = X.vector_of(b, [-int(v) for v in P["coef"][0]], [-int(v) for v in t])  # -(coef b) + t
    assert max(abs(v) for v in t_red) < 2**53
    c = _gscoords(b, mu, rd, t_red)
    assert np.array_equal(c.view(np.uint64), P["target_coord"][0].view(np.uint64))


# ---- the C ABI, the build, the wrappers ------------------------------------------------------------------------------
def test_the_c_abi_has_the_route_call(tmp_path):
    from fplll_amd import _lib
    lib = _lib.load()
    assert lib.fphip_abi_version() >= 7
    fn = _lib.bind_closest_vector_ex(lib)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert _lib.CVP_ROUTES == {"auto": 0, "wave": 1, "enum": 2} and _lib.CVP_NODE_LIMIT == 2
    assert fn(None, None, 0, 1, None, 0, 0, 0, None, None, None, None, None) == -1  # no object: nothing dereferenced
    hdr = os.path.join(C.ROOT, "include", "fplll_hip.h")
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n'
                   'int (*p)(fphip_gso *, fphip_ctx *, int, int, const int64_t *, int, int, uint64_t, int64_t *, double *,\n'
                   '         int64_t *, uint64_t *, int *) = fphip_closest_vector_ex;\n'
                   'int v[] = {FPHIP_CVP_ROUTE_AUTO, FPHIP_CVP_ROUTE_WAVE, FPHIP_CVP_ROUTE_ENUM, FPHIP_CVP_NODE_LIMIT,\n'
                   '           FPHIP_CVPM_FAST, FPHIP_CVPM_PROVED};\n' % hdr)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_build_lists_the_kernel_with_the_flag_of_its_twin():
    from fplll_amd import build
    assert "cvp_wave.hip" in build.HIP_SOURCES
    assert build.PER_FILE_FLAGS["cvp_wave.hip"] == build.PER_FILE_FLAGS["svp_wave.hip"]


LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")
def test_wave_kernels_of_all_four_widths_compile_without_scratch(tmp_path):
    """cvp_wave_kernel<1..4> are in the code object build() left behind, each without scratch memory and within the
    128 registers svp_wave_kernel is held to (DESIGN section 3g records the figures as built)."""
    from fplll_amd import build
    build.build_hip()
    obj = os.path.join(C.ROOT, "fplll_amd", "lib", "obj", "cvp_wave.hip.o")
    assert os.path.exists(obj), obj
    fat, co = str(tmp_path / "cvp.fat"), str(tmp_path / "cvp.co")
    subprocess.check_call([TOOLS[0], "--dump-section", ".hip_fatbin=" + fat, obj, str(tmp_path / "unused.o")])
    subprocess.check_call([TOOLS[1], "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([TOOLS[2], "--notes", co]).decode()
    seen = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        seen[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                      int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    want = ["_ZN5fphip15cvp_wave_kernelILi%dEEEvNS_8GsoBatchENS_7CvpWaveE" % nq for nq in (1, 2, 3, 4)]
    assert sorted(seen) == want, sorted(seen)
    for k, (regs, scratch) in seen.items():
        assert scratch == 0 and regs <= 128, (k, regs, scratch)


def test_wrappers_check_the_route_before_anything_else():
    """Every check comes before the context or the device object is touched (None / a bare object here)."""
    from fplll_amd.cvp import closest_vector, closest_vectors
    from fplll_amd.gso import MatGSOBatch
    b = np.eye(3, dtype=np.int64)
    with pytest.raises(ValueError, match="route is one of auto, enum, wave"):
        closest_vector(None, b, np.zeros(3, dtype=np.int64), route="fastest")
    with pytest.raises(ValueError, match="route is one of auto, enum, wave"):
        closest_vectors(None, b, np.zeros((2, 3), dtype=np.int64), route=1)
    with pytest.raises(ValueError, match="max_nodes"):
        closest_vectors(None, b, np.zeros((2, 3), dtype=np.int64), route="wave", max_nodes=-1)
    with pytest.raises(ValueError, match="route is one of auto, enum, wave"):
        MatGSOBatch.closest_vector(object(), np.zeros((2, 3), dtype=np.int64), route="gpu")
    with pytest.raises(ValueError, match="max_nodes"):
        MatGSOBatch.closest_vector(object(), np.zeros((2, 3), dtype=np.int64), route="auto", max_nodes=-5)
