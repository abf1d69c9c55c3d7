"""CPU side of the transformation matrix on the Householder objects (fphip_hh_enable_transform): the reference the GPU
tests compare u with is sound on every input they use, the u-carrying kernels live in their own code objects within
the plain kernels' register classes, and the C ABI declares the two entry points.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import conftest as C
import hlll_transform_cases as T
import wide_cases as W
from test_abi import declared_symbols

CASES = list(T.soundness_cases())


# ---- 1. the checker ----------------------------------------------------------------------------------------------------
def test_the_inputs_are_the_ones_named():
    names = [c[0] for c in CASES]
    assert names[:5] == list(T.HLLL_FIXTURES)
    assert sum(n.startswith("hhsr_") for n in names) == 4
    assert sum(n.startswith("short") for n in names) == len(W.SHORT_WIDE) * W.SHORT_BATCH
    assert sum(n.startswith("tall180") for n in names) == 3 and sum(n.startswith("tall200") for n in names) == 3


@pytest.mark.parametrize("name,b_in,b_out", CASES, ids=[c[0] for c in CASES])
def test_reference_transform_is_unique_integral_and_unimodular(name, b_in, b_out):
    """U b_in = b_out has ONE solution (b_in has full row rank), it is an integer matrix, and |det U| = 1 — so the
    reference's u is that matrix and nothing else.  Up to 72 rows by wide_cases.solve_left_exact (None would mean a
    rank-deficient input); on square inputs also — and beyond 72 rows, where the elimination takes minutes, only — by
    the verified proposal of hlll_transform_cases.transform_by_verification, and where both run they must agree."""
    d, n = b_in.shape
    U = None
    if d <= 72:
        sol = W.solve_left_exact(b_in, b_out)
        assert sol is not None, "rank-deficient input: the transformation is not unique"
        num, den = sol
        assert den > 0 and all(v % den == 0 for row in num for v in row)
        U = np.array([[v // den for v in row] for row in num], dtype=object)
    if d == n:
        V = T.transform_by_verification(b_in, b_out)
        assert U is None or np.array_equal(U, V)
        U = V
    assert U is not None
    assert W._matmul_equals(U, b_in.astype(object), b_out.astype(object))
    assert abs(W.bareiss_det(U)) == 1
    assert T.is_unimodular(U.astype(np.int64))
    assert np.array_equal(T.unique_transform(b_in, b_out), U)


def test_the_checker_rejects_what_it_must():
    f = T.hlll_fixture("hlll_u24")
    b_in, b_out = f["b_in"], f["b_out"]
    U = T.unique_transform(b_in, b_out).astype(np.int64)
    T.check_transform(U, b_in, b_out)
    bad = U.copy()
    bad[3, 5] += 1
    with pytest.raises(AssertionError):
        T.check_transform(bad, b_in, b_out)
    # a rank-deficient input has no unique transformation: the elimination says so, and so does the residue test
    dup = b_in.copy()
    dup[7] = dup[2]
    assert W.solve_left_exact(dup, dup) is None
    assert not T.nonsingular_mod_p(dup) and T.nonsingular_mod_p(b_in)
    with pytest.raises(AssertionError):
        T.transform_by_verification(dup, dup)
    # not unimodular
    assert not T.is_unimodular(2 * np.eye(60, dtype=np.int64)) and not T.is_unimodular(2 * np.eye(5, dtype=np.int64))
    for d in (8, 60):
        u0 = T.seeded_unimodular(d, 1)
        assert T.is_unimodular(u0) and not np.array_equal(u0, np.eye(d, dtype=np.int64)) and np.abs(u0).max() <= 64


# ---- 2. the code objects (the approach of tests/test_kernel_budgets.py) ------------------------------------------------
LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
needs_llvm = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")

# registers per lane for N resident waves per SIMD (512 per lane, allocated in eights)
WAVES = {8: 64, 5: 96, 4: 128, 3: 168, 2: 256}


def _kernels(src, tmp):
    """{mangled kernel name: (registers = VGPRs + AGPRs, scratch bytes per lane)} of one translation unit."""
    from fplll_amd import build
    build.build_hip()
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


def _pick(ks, pattern):
    hit = {k: v for k, v in ks.items() if re.search(pattern, k)}
    assert hit, pattern
    return hit


@needs_llvm
def test_u_kernels_live_in_their_own_code_object_within_the_plain_wave_classes(tmp_path):
    """hlll_u_kernel<1..4> come out of hlll_kernel_u.hip, nothing of them out of hlll_kernel.hip (whose kernels the
    occupancy of the plain HLLL rests on, tests/test_kernel_budgets.py), and they keep the plain kernel's waves per
    SIMD — 5 / 4 / 3 / 2 for NQ 1 .. 4 — with nothing in scratch memory (the ring's waits count every vector-memory
    instruction: a spill inside a phase would break them)."""
    ku = _kernels("hlll_kernel_u.hip", str(tmp_path))
    for nq, top in {1: WAVES[5], 2: WAVES[4], 3: WAVES[3], 4: WAVES[2]}.items():
        (k, (regs, scratch)), = _pick(ku, r"hlll_u_kernelILi%dE" % nq).items()
        assert regs <= top and scratch == 0, (k, regs, top, scratch)
    assert not [k for k in ku if re.search(r"hlll_kernelILi", k)]
    kp = _kernels("hlll_kernel.hip", str(tmp_path))
    assert not [k for k in kp if "_u_" in k], sorted(kp)
    assert len(_pick(kp, r"hlll_kernelILi\dE")) == 4


@needs_llvm
def test_extended_precision_and_size_reduce_twins(tmp_path):
    """hlll_x_u_kernel<NQ, FT> is the output of hlll_x_u.hip alone (twelve instantiations, none of them in hlll_x.hip,
    and no second copy of the unit-test kernels); hh_size_reduce_u_kernel sits next to hh_size_reduce_kernel, both
    without scratch memory."""
    kx, kxu = _kernels("hlll_x.hip", str(tmp_path)), _kernels("hlll_x_u.hip", str(tmp_path))
    assert len(_pick(kxu, r"hlll_x_u_kernelILi\dE")) == 12 and len(kxu) == 12
    assert len(_pick(kx, r"hlll_x_kernelILi\dE")) == 12 and not [k for k in kx if "_u_" in k]
    for ft in ("d", "NS_2DDE"):   # (the quad-double instantiations spill in the plain kernel already)
        for k, (regs, scratch) in _pick(kxu, r"hlll_x_u_kernelILi\dE%sEE" % ft).items():
            assert scratch == 0, (k, scratch)
    kr = _kernels("hh_rows.hip", str(tmp_path))
    for pat in (r"hh_size_reduce_kernel", r"hh_size_reduce_u_kernel"):
        (k, (regs, scratch)), = _pick(kr, pat).items()
        assert regs <= WAVES[8] and scratch == 0, (k, regs, scratch)


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------
def test_abi_declares_the_transform_pair():
    syms = declared_symbols()
    assert "fphip_hh_enable_transform" in syms and "fphip_hh_get_transform" in syms
    hdr = open(os.path.join(C.ROOT, "include", "fplll_hip.h")).read()
    assert re.search(r"int\s+fphip_hh_enable_transform\(fphip_hh \*h, const int64_t \*u\);", hdr)
    assert re.search(r"int\s+fphip_hh_get_transform\(fphip_hh \*h, int first, int count, int64_t \*u\);", hdr)


def test_python_layer_has_the_three_methods():
    from fplll_amd.householder import MatHouseholderBatch
    for m in ("enable_transform", "get_transform", "get_inverse_transform_t"):
        assert callable(getattr(MatHouseholderBatch, m, None)), m
    assert "started at the identity" in " ".join(MatHouseholderBatch.get_inverse_transform_t.__doc__.split())
