"""Closest-vector mode of the enumeration (enumerate_block(..., target=t), fphip_enum_opts::target), the CPU half: the
exact rational reference tests/exact_cvp.py against the shortest-vector one it is modelled on, the sizes of the named
blocks the GPU tests run, the new field of the C ABI, and the register / scratch budget of the kernels compiled for
the mode.  No GPU.

The named blocks (exact_cvp.CVP_BLOCKS), exact reference at the radius of the table:

  name    d   R     nodes  candidates  k0  max children  half-int centres  integer centres  at the bound
  dy12t   12  1.25   8784     994      0       5            2120              2498             142
  dy20t   20  1.0    5581      10      2       4            1174              1506               1
  pr28t   28  1.25   8142      50      4       3            2060              2102               7
  q2t     16  2.0   14384    1212      0       5            6970              7414             514
  z8t      8  4.0    4096    2304      0       4            4096                 0            2048
"""
import os
import re
import subprocess

import numpy as np
import pytest

import conftest as C
import exact_cvp as X
import exact_enum as E


@pytest.mark.parametrize("name", ["eq10", "dy12", "z8"])
def test_zero_target_is_the_mirrored_half_tree(name):
    """An all-zero target: the closest-vector tree is the shortest-vector half tree and its mirror image, glued at the
    all-zero prefix.  Every candidate x of exact_enumerate comes with -x, plus the zero vector at distance 0; per level
    the plain count is twice the shortest-vector count of non-zero prefixes plus the zero prefix."""
    mut, rdiag, pruning, R = E.TIE_BLOCKS[name]()
    d = len(rdiag)
    nodes_s, cands_s, _ = E.exact_enumerate(mut, rdiag, pruning, R, max_nodes=30000)
    nodes_c, cands_c, stats = X.exact_cvp_enumerate(mut, rdiag, pruning, R, np.zeros(d), max_nodes=60000)
    want = [(a, x) for a, x in cands_s] + [(a, tuple(-v + 0.0 for v in x)) for a, x in cands_s] + [(0.0, (0.0,) * d)]
    assert sorted(want) == cands_c
    # exact_enumerate: the zero prefix is not counted at the levels >= 1 and is counted at level 0
    assert stats["plain"] == [2 * (nodes_s[0] - 1) + 1] + [2 * nodes_s[k] + 1 for k in range(1, d)]
    # the rounding descent is the zero vector: it never leaves the radius, every level above 0 loses one node
    assert stats["k0"] == 0
    assert nodes_c == [stats["plain"][0]] + [2 * nodes_s[k] for k in range(1, d)] + [0]


@pytest.mark.parametrize("name", list(X.CVP_BLOCKS))
def test_named_blocks_are_small_and_full_of_ties(name):
    """Every named block has between 2 000 and 30 000 exact nodes (what keeps this file under a minute and each GPU
    case at a few seconds), candidates, and the ties it is named for."""
    nodes, cands, stats = X.exact_of(name)
    total = sum(stats["plain"])
    assert 2000 <= total <= 30000, total
    assert len(cands) >= 10 and stats["at_bound"] >= 1
    assert stats["half_centres"] >= 1000
    assert cands == sorted(cands) and len(set(cands)) == len(cands)
    if name == "z8t":
        assert stats["min_group"] == 256 and cands[0][0] == 2.0 and stats["half_centres"] == total
    if name == "q2t":
        assert stats["half_centres"] + stats["int_centres"] == total
    if name in ("dy20t", "pr28t"):
        assert stats["k0"] > 0  # the rounding descent leaves the radius: fewer levels are compensated


def test_lattice_point_target_is_found_at_distance_zero():
    """A target that IS a lattice point: the zero leaf is a candidate (distance exactly 0), and x and its neighbours
    on the other side of the target are both there (no half tree)."""
    mut, rdiag = E.dyadic_block(10, 3, q=4, rexp=(0,))
    x = np.array([1.0, -2.0, 0.0, 3.0, 0.0, 0.0, -1.0, 0.0, 2.0, -1.0])
    target = np.array([x[i] + sum(x[j] * mut[i, j] for j in range(i + 1, 10)) for i in range(10)])
    nodes, cands, stats = X.exact_cvp_enumerate(mut, rdiag, None, 1.0, target, max_nodes=30000)
    assert cands[0] == (0.0, tuple(x)) and stats["min_group"] == 1 and stats["k0"] == 0
    rel = sorted(tuple(v - w for v, w in zip(c, x)) for _, c in cands)
    assert rel == sorted(tuple(-v + 0.0 for v in r) for r in rel)  # symmetric about the lattice point


def test_enum_opts_has_the_target_field(tmp_path):
    """The C ABI: `target` is the LAST field of fphip_enum_opts, in the header and in the ctypes mirror, at the same
    offset; the header still compiles as C."""
    from fplll_amd import _lib
    assert _lib.EnumOpts._fields_[-1][0] == "target"
    assert _lib.EnumOpts.target.size == 8
    hdr = os.path.join(C.ROOT, "include", "fplll_hip.h")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu\\n", '
                   'offsetof(fphip_enum_opts, target), sizeof(fphip_enum_opts)); return 0; }\n' % hdr)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    off, size = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert off == _lib.EnumOpts.target.offset and size == __import__("ctypes").sizeof(_lib.EnumOpts)
    assert off + 8 == size  # the last field
    assert _lib.load().fphip_abi_version() >= 3


LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")
def test_cvp_phase_kernels_keep_their_budget(tmp_path):
    """The closest-vector instantiations of the split / overflow walk meet the budget of their shortest-vector twins
    (test_kernel_budgets.py): at most 64 registers per lane — 8 waves per SIMD — and nothing in scratch memory.  Read
    off the metadata of the code object build() left behind."""
    from fplll_amd import build
    build.build_hip()
    obj = os.path.join(C.ROOT, "fplll_amd", "lib", "obj", "enum_kernel_cvp.hip.o")
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
    phase = {k: v for k, v in seen.items() if "enum_phase_cvp_kernel" in k}
    assert len(phase) == 2, sorted(seen)  # <MU_LDS = true / false, SUBS = false, DUAL = false>
    for k, (regs, scratch) in phase.items():
        assert regs <= 64 and scratch == 0, (k, regs, scratch)
    # the translation unit holds the closest-vector kernels and nothing else: the kernels of the shortest-vector walk
    # are compiled once, from enum_kernel.hip
    assert all("_cvp_kernel" in k for k in seen), sorted(seen)
