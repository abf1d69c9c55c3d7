"""List mode of the enumeration (fphip_enum_list), the CPU half: the kernels compiled for the mode —
their names, their register and scratch budgets read from the objects build() left behind — the canonical order of
the host (fphip_list_sort_records needs no device), the new entry points of the C ABI, and the argument checks of
enumeration.list_block.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import conftest as C

LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
needs_tools = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")
# names that the static guards of the other modes select their kernels by: no list kernel may match one
TWIN_NAMES = ("enum_walk_kernel", "enum_walk_cvp_kernel", "enum_phase_kernel", "enum_phase_cvp_kernel")
_seen = {}


def _kernels(source, tmp):
    """{kernel name: (vgprs, scratch bytes)} of the gfx950 code object of one translation unit."""
    if source not in _seen:
        from fplll_amd import build
        build.build_hip()
        obj = os.path.join(C.ROOT, "fplll_amd", "lib", "obj", source + ".o")
        assert os.path.exists(obj), obj
        fat, co = os.path.join(tmp, source + ".fat"), os.path.join(tmp, source + ".co")
        subprocess.check_call([TOOLS[0], "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "unused.o")])
        subprocess.check_call([TOOLS[1], "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([TOOLS[2], "--notes", co]).decode()
        out = {}
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            out[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                         int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
        _seen[source] = out
    return _seen[source]


def _template_args(name):
    return re.search(r"kernelI(\w+?)EEv", name).group(1)


@needs_tools
@pytest.mark.parametrize("source,kernel", [("enum_kernel_list.hip", "enum_phase_list_kernel"),
                                           ("enum_kernel_cvp_list.hip", "enum_phase_cvp_list_kernel")])
def test_list_phase_kernels_keep_their_budget(tmp_path, source, kernel):
    """The list instantiations of the split / overflow walk meet the budget of their twins: at most 64 registers per
    lane and nothing in scratch memory; the translation unit holds them and nothing else."""
    seen = _kernels(source, str(tmp_path))
    assert len(seen) == 2 and all(kernel in k for k in seen), sorted(seen)  # <MU_LDS = true / false, false, false>
    for k, (regs, scratch) in seen.items():
        assert regs <= 64 and scratch == 0, (k, regs, scratch)


@needs_tools
@pytest.mark.parametrize("source,kernel,twin", [("enum_walk_list.hip", "enum_walk_list_kernel", "enum_walk.hip"),
                                                ("enum_walk_cvp_list.hip", "enum_walk_cvp_list_kernel",
                                                 "enum_walk_cvp.hip")])
def test_list_walk_kernels_use_no_more_scratch_than_their_twins(tmp_path, source, kernel, twin):
    seen = _kernels(source, str(tmp_path))
    twins = {_template_args(k): v for k, v in _kernels(twin, str(tmp_path)).items()}
    assert len(seen) == 4 and all(kernel in k for k in seen), sorted(seen)  # <MU_LDS, DUAL = false, CHAIN>
    for k, (regs, scratch) in seen.items():
        assert regs <= 64 and scratch <= twins[_template_args(k)][1], (k, regs, scratch, twins[_template_args(k)])


@needs_tools
def test_list_kernel_names_match_no_guard_of_the_other_modes(tmp_path):
    names = []
    for source in ("enum_kernel_list.hip", "enum_kernel_cvp_list.hip", "enum_walk_list.hip", "enum_walk_cvp_list.hip"):
        names += list(_kernels(source, str(tmp_path)))
    assert len(names) == 12
    for n in names:
        assert "_list_kernel" in n and not any(t in n for t in TWIN_NAMES), n
    # and the four existing translation units hold no list kernel
    for source in ("enum_kernel.hip", "enum_kernel_cvp.hip", "enum_walk.hip", "enum_walk_cvp.hip"):
        assert not any("_list_kernel" in k for k in _kernels(source, str(tmp_path)))


def test_build_lists_the_new_translation_units_like_their_twins():
    from fplll_amd import build
    for new, twin, text in (("enum_kernel_list.hip", "enum_kernel.hip", "enum_kernel.hip"),
                            ("enum_kernel_cvp_list.hip", "enum_kernel_cvp.hip", "enum_kernel.hip"),
                            ("enum_walk_list.hip", "enum_walk.hip", "enum_walk.hip"),
                            ("enum_walk_cvp_list.hip", "enum_walk_cvp.hip", "enum_walk.hip")):
        assert new in build.HIP_SOURCES
        assert build.PER_FILE_FLAGS[new] == build.PER_FILE_FLAGS[twin]
        assert build.EXTRA_DEPS[new] == [text]
        src = open(os.path.join(build.CSRC, new)).read()
        code = [l for l in src.split("\n") if l.strip() and not l.startswith("//")]
        assert code[-1] == '#include "%s"' % text and "#define FPHIP_LIST 1" in code[:-1] and len(code) <= 3


def _sort(dim, dist, x):
    from fplll_amd import _lib
    lib = _lib.load()
    lib.fphip_list_sort_records.argtypes = [ctypes.c_int, ctypes.c_uint64] + [ctypes.c_void_p] * 4
    lib.fphip_list_sort_records.restype = None
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(len(dist), dim)
    do, xo = np.full(len(dist) + 2, -7.5), np.full((len(dist) + 2, dim), -7.5)
    lib.fphip_list_sort_records(dim, len(dist), dist.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p),
                                do.ctypes.data_as(ctypes.c_void_p), xo.ctypes.data_as(ctypes.c_void_p))
    assert (do[len(dist):] == -7.5).all() and (xo[len(dist):] == -7.5).all()  # nothing behind the n records
    return do[:len(dist)], xo[:len(dist)]


def test_canonical_sort_of_the_host():
    """Distance ascending; ties by the coefficients compared from the TOP level down; any input order, one output."""
    rng = np.random.default_rng(5)
    dim, n = 5, 400
    x = rng.integers(-2, 3, size=(n, dim)).astype(np.float64)
    x = np.unique(x, axis=0)
    n = len(x)
    dist = rng.integers(1, 4, size=n).astype(np.float64)  # three distances: long runs of ties
    want = sorted(zip(dist.tolist(), [tuple(r) for r in x.tolist()]), key=lambda t: (t[0], t[1][::-1]))
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(n)
        do, xo = _sort(dim, dist[p], x[p])
        assert list(zip(do.tolist(), [tuple(r) for r in xo.tolist()])) == want
    # level 1 (the top one of two) is compared before level 0
    do, xo = _sort(2, [1.0, 1.0, 0.5], [[5.0, 0.0], [-3.0, 1.0], [9.0, 9.0]])
    assert do.tolist() == [0.5, 1.0, 1.0] and xo.tolist() == [[9.0, 9.0], [5.0, 0.0], [-3.0, 1.0]]
    assert _sort(3, [], np.zeros((0, 3)))[0].size == 0


def test_the_c_abi_has_the_list_entry_points(tmp_path):
    from fplll_amd import _lib
    lib = _lib.load()
    assert lib.fphip_abi_version() >= 5
    assert hasattr(lib, "fphip_enum_list") and hasattr(lib, "fphip_list_sort_records")
    hdr = os.path.join(C.ROOT, "include", "fplll_hip.h")
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n'
                   'int (*p)(fphip_ctx *, int, double, const double *, const double *, const double *, const double *,\n'
                   '         uint64_t, double *, double *, uint64_t *, uint64_t *, fphip_enum_stats *) = fphip_enum_list;\n'
                   'void (*q)(int, uint64_t, const double *, const double *, double *, double *) = '
                   'fphip_list_sort_records;\n' % hdr)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_list_block_checks_its_arguments():
    """Every check comes before the context is touched (ctx = None here)."""
    from fplll_amd.enumeration import Unsupported, list_block
    mut, r = np.zeros((4, 4)), np.ones(4)
    with pytest.raises(ValueError, match="square"):
        list_block(None, np.zeros(7), r, None, 1.0)
    with pytest.raises(ValueError, match="rdiag"):
        list_block(None, mut, np.ones(3), None, 1.0)
    with pytest.raises(ValueError, match="pruning"):
        list_block(None, mut, r, np.ones(5), 1.0)
    with pytest.raises(ValueError, match="target"):
        list_block(None, mut, r, None, 1.0, target=np.zeros(3))
    with pytest.raises(ValueError, match="cap"):
        list_block(None, mut, r, None, 1.0, cap=-1)
    with pytest.raises(ValueError, match="radius"):
        list_block(None, mut, r, None, float("nan"))
    with pytest.raises(Unsupported, match="several ranks"):
        list_block(None, mut, r, None, 1.0, shard_count=2)


def test_svp_wrappers_check_their_arguments():
    """fplll_amd.svp: shapes, the bound and the capacity are checked before anything touches a device (ctx = None)."""
    import fplll_amd
    from fplll_amd.svp import short_vectors, theta_series, vectors_near
    assert fplll_amd.short_vectors is short_vectors and fplll_amd.vectors_near is vectors_near
    assert fplll_amd.theta_series is theta_series
    b = np.eye(4, dtype=np.int64)
    with pytest.raises(ValueError, match=r"b is \[d\]\[n\]"):
        short_vectors(None, np.zeros(4, dtype=np.int64), 2)
    with pytest.raises(ValueError, match=r"b is \[d\]\[n\]"):
        short_vectors(None, np.zeros((5, 4), dtype=np.int64), 2)
    with pytest.raises(ValueError, match="bound_sq"):
        short_vectors(None, b, -1)
    with pytest.raises(ValueError, match="bound_sq"):
        short_vectors(None, b, 2.5)
    with pytest.raises(ValueError, match="cap"):
        short_vectors(None, b, 2, cap=-1)
    with pytest.raises(ValueError, match="target"):
        vectors_near(None, b, np.zeros(3, dtype=np.int64), 2)
