"""Closest-vector enumeration of blocks above 64 rows, the CPU half: the conditions of the recorded fixtures
tests/golden/cvpw_*.json.gz, the sizes of the exact dyadic blocks the GPU tests run (tests/wide_cvp_cases.py), and the
register / scratch budget of the top walk compiled for the mode.  No GPU.

  fixture            d    nodes   largest level >= 64   level 64   candidates   k0
  cvpw_d72_real      72   957259        1078               1078        2        20
  cvpw_d72_lattice   72    27657        1040               1040        1         0
  cvpw_d96_k0        96    56378        5054                 58        1        65
  cvpw_d136_k0      136    54857        5106                  1        1        93
"""
import os
import re
import subprocess

import pytest

import conftest as C
import wide_cvp_cases as W


def _signed(v):
    return v - 2**64 if v >= 2**63 else v  # (a level the reference's unchecked decrement wrapped reads 2^64 - 1)


def test_the_fixture_set():
    assert W.FIXTURES == ["cvpw_d136_k0", "cvpw_d72_lattice", "cvpw_d72_real", "cvpw_d96_k0"]
    largest_before = 310200  # tests/golden/gso_q64_p5.json, the largest file there before these
    for n in W.FIXTURES:
        assert os.path.getsize(os.path.join(C.GOLDEN, n + ".json.gz")) <= largest_before
    descs = {n: W.fixture(n)["desc"] for n in W.FIXTURES}
    assert "radius=gh:" in descs["cvpw_d72_real"] and "target=real" in descs["cvpw_d72_real"]
    assert "target=lattice" in descs["cvpw_d72_lattice"]
    for n in ("cvpw_d96_k0", "cvpw_d136_k0"):
        f = float(re.search(r"radius=babai:(\S+)", descs[n]).group(1))
        assert f < 1.0
    assert sorted(W.fixture(n)["d"] for n in W.FIXTURES) == [72, 72, 96, 136]  # NQT = 2, 2, 2 and 4


@pytest.mark.parametrize("name", W.FIXTURES)
def test_fixture_conditions(name):
    """(a) 10^4 .. 3 10^6 nodes in all; (b) a level >= 64 with at least 3 nodes, level 64 within the top task buffer;
    (c) a candidate; (d) the shortest candidate is alone at its distance, is what the reference's BEST_N(1) run ended
    on, and passes every pruned bound under its own distance."""
    f = W.fixture(name)
    d = f["d"]
    nodes = [_signed(v) for v in f["nodes"]]
    assert 10**4 <= sum(nodes) <= 3 * 10**6
    assert max(nodes[64:d]) >= 3 and nodes[64] <= W.TOP_TASK_CAP
    assert len(f["cands"]) >= 1
    m, xm = f["cands"][0]
    assert f["best"] == (m, xm) and (len(f["cands"]) == 1 or f["cands"][1][0] > m)
    assert W.safe_under_own_distance(f, m, xm)


def test_descent_stops():
    """k0 > 0 where the radius is a fraction of the descent's distance, >= 64 in two fixtures (the compensation of the
    levels >= 64 stops short), 0 for the lattice point; the lattice point is at distance exactly 0."""
    k0 = {n: W.descent_stop(W.fixture(n)) for n in W.FIXTURES}
    assert k0 == {"cvpw_d136_k0": 93, "cvpw_d72_lattice": 0, "cvpw_d72_real": 20, "cvpw_d96_k0": 65}
    f = W.fixture("cvpw_d72_lattice")
    assert f["best"] == (0.0, tuple([0.0] * 71 + [3.0]))
    # the reference took one node off the levels k0 < i < d only: the levels below k0 it reached hold plain counts
    for n in ("cvpw_d96_k0", "cvpw_d136_k0"):
        f = W.fixture(n)
        assert all(_signed(v) >= 0 for v in f["nodes"])


@pytest.mark.parametrize("name", list(W.WIDE_BLOCKS))
def test_exact_wide_blocks_are_narrow_and_branch_above_64(name):
    """The exact reference stays under 3 10^4 nodes, the levels >= 64 branch, and four closest vectors tie."""
    nodes, cands, stats = W.exact_of(name)
    d = W.WIDE_BLOCKS[name][0]
    assert 2000 <= sum(stats["plain"]) <= 30000
    assert max(stats["plain"][64:d]) >= 100 and stats["plain"][64] <= W.TOP_TASK_CAP
    assert stats["min_group"] == 4 and len(cands) >= 10 and stats["half_centres"] >= 50
    assert any(any(v != 0.0 for v in x[64:]) for _, x in cands)


LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]


def _kernels(obj, tmp_path, tag):
    fat, co = str(tmp_path / (tag + ".fat")), str(tmp_path / (tag + ".co"))
    subprocess.check_call([TOOLS[0], "--dump-section", ".hip_fatbin=" + fat, obj, str(tmp_path / (tag + ".unused.o"))])
    subprocess.check_call([TOOLS[1], "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([TOOLS[2], "--notes", co]).decode()
    seen = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        seen[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                      int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return seen


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")
def test_cvp_top_kernels_keep_their_twins_budget(tmp_path):
    """enum_top_cvp_kernel<2 / 4, false, false>: no more registers than enum_top_kernel<2 / 4, false, false> and
    nothing in scratch memory.  Read off the metadata of the code objects build() left behind."""
    from fplll_amd import build
    build.build_hip()
    objdir = os.path.join(C.ROOT, "fplll_amd", "lib", "obj")
    cvp = {k: v for k, v in _kernels(os.path.join(objdir, "enum_kernel_cvp.hip.o"), tmp_path, "cvp").items()
           if "enum_top_cvp_kernel" in k}
    svp = {k: v for k, v in _kernels(os.path.join(objdir, "enum_kernel.hip.o"), tmp_path, "svp").items()
           if "enum_top_kernel" in k}
    assert len(cvp) == 2 and len(svp) == 6, (sorted(cvp), sorted(svp))
    for nqt in (2, 4):
        tag = "ILi%dELb0ELb0EE" % nqt
        (regs, scratch), = [v for k, v in cvp.items() if tag in k]
        (regs0, scratch0), = [v for k, v in svp.items() if tag in k]
        assert scratch == 0 and scratch0 == 0 and regs <= regs0, (nqt, regs, regs0)
