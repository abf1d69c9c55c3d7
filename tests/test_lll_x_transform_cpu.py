"""CPU side of the transformation matrix under lll_ex / lll_ladder (lll_x_u.hip): the u-carrying kernels are the
output of their own translation unit and lll_x.hip still yields the twelve plain ones alone, their registers and
scratch memory stay within the figures measured when they were written (profiles/lll_x_transform.md), and
gso.lll_reduction refuses what the device does not cover before it touches one.  No GPU."""
import os
import re
import subprocess

import pytest

import conftest as C

LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
needs_llvm = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="needs the ROCm LLVM tools")

FT = {"double": "d", "DD": "NS_2DDE", "QD": "NS_2QDE"}
U_KERNELS = [(nq, ft) for ft in ("double", "DD") for nq in (1, 2, 3, 4)] + [(1, "QD")]
PLAIN_KERNELS = [(nq, ft) for ft in ("double", "DD", "QD") for nq in (1, 2, 3, 4)]


def _kernels(src, tmp):
    """{mangled kernel name: (registers = VGPRs + AGPRs, scratch bytes per lane)} of one translation unit, from the
    metadata of its gfx950 code object (the approach of tests/test_kernel_budgets.py)"""
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


def _plain(nq, ft):
    return "_ZN5fphip12lll_x_kernelILi%dE%sEEvNS_4LllXE" % (nq, FT[ft])


def _tracked(nq, ft):
    # (LllX, long long *, long long *, int): the second pointer is a substitution of the first
    return "_ZN5fphip14lll_x_u_kernelILi%dE%sEEvNS_4LllXEPxS%s_i" % (nq, FT[ft], "2" if ft == "double" else "3")


# ---- 1. the kernel names -------------------------------------------------------------------------------------------------
@needs_llvm
def test_each_translation_unit_holds_its_own_kernels_and_no_others(tmp_path):
    """lll_x_u.hip: exactly the nine lll_x_u_kernel instantiations (1 .. 4 columns per lane in double and
    double-double, one in quad-double); lll_x.hip: the twelve lll_x_kernel instantiations and nothing of the twin."""
    ku, kp = _kernels("lll_x_u.hip", str(tmp_path)), _kernels("lll_x.hip", str(tmp_path))
    assert sorted(ku) == sorted(_tracked(nq, ft) for nq, ft in U_KERNELS)
    assert sorted(kp) == sorted(_plain(nq, ft) for nq, ft in PLAIN_KERNELS)
    assert not [k for k in kp if "lll_x_u_kernel" in k] and not [k for k in ku if "lll_x_kernelI" in k]


# ---- 2. registers and scratch memory -------------------------------------------------------------------------------------
# VGPRs + AGPRs and scratch bytes per lane of every u instantiation as the cross-compile for gfx950 gave them when the
# kernel was written (profiles/lll_x_transform.md has them next to the plain twins'): upper bounds from here on.
# The launch keeps at most two waves per SIMD resident (a grid of eight one-wave blocks per CU), which every one of
# them allows (256 registers); the scratch bytes are those of the plain twin (its lane-indexed arrays), none is added.
U_BUDGET = {(1, "double"): (106, 0), (2, "double"): (115, 0), (3, "double"): (125, 0), (4, "double"): (135, 0),
            (1, "DD"): (123, 0), (2, "DD"): (129, 0), (3, "DD"): (139, 256), (4, "DD"): (149, 256),
            (1, "QD"): (169, 272)}
TWO_WAVES = 256   # registers per lane with which two waves per SIMD stay resident


@needs_llvm
def test_u_kernels_stay_within_the_measured_registers_and_scratch(tmp_path):
    ku, kp = _kernels("lll_x_u.hip", str(tmp_path)), _kernels("lll_x.hip", str(tmp_path))
    assert sorted(U_BUDGET) == sorted(U_KERNELS)
    for (nq, ft), (regs_top, scratch_top) in U_BUDGET.items():
        regs, scratch = ku[_tracked(nq, ft)]
        assert regs <= regs_top and scratch <= scratch_top, (nq, ft, regs, scratch)
        assert regs <= TWO_WAVES
        assert scratch <= kp[_plain(nq, ft)][1], (nq, ft, scratch, kp[_plain(nq, ft)])   # no scratch the twin has not


# ---- 3. the public entry ---------------------------------------------------------------------------------------------------
class _NoDevice:
    """stands where the context goes: any use of it is a device call"""

    def __getattr__(self, name):
        raise AssertionError("lll_reduction touched the device (%s) before refusing" % name)


@pytest.mark.parametrize("kwargs", [dict(method="proved"), dict(method="heuristic"), dict(method="LM_FAST"),
                                    dict(method="fast", float_type="mpfr"), dict(method="fast", float_type="long double"),
                                    dict(method="fast", float_type="dpe"), dict(method="fast", float_type=106),
                                    dict(method="wrapper", float_type="dd"), dict(method="wrapper", float_type="mpfr")])
def test_lll_reduction_refuses_what_the_device_does_not_cover(kwargs):
    import numpy as np
    from fplll_amd import gso
    with pytest.raises(ValueError, match="lll_reduction"):
        gso.lll_reduction(_NoDevice(), np.eye(4, dtype=np.int64), **kwargs)


def test_the_docstrings_say_that_u_is_carried():
    from fplll_amd import gso
    flat = lambda f: " ".join(f.__doc__.split())  # noqa: E731
    assert "transformation matrix u is carried" in flat(gso.MatGSOBatch.lll_ex)
    assert "transformation matrix u is carried" in flat(gso.MatGSOBatch.lll_ladder)
    assert "u is carried by lll_ex()" in flat(gso.MatGSOBatch.enable_transform)
    assert "lll_ladder()" in flat(gso.MatGSOBatch.enable_transform)
    for f in (gso.MatGSOBatch.lll_ex, gso.MatGSOBatch.lll_ladder, gso.MatGSOBatch.enable_transform):
        assert "max(d, n) <= 64" in flat(f) or "max(d, n) > 64" in flat(f)   # the quad-double limit
    for word in ('"fast"', '"wrapper"', '"dd"', '"qd"', "ValueError"):
        assert word in flat(gso.lll_reduction), word


def test_the_header_describes_the_new_contract():
    hdr = " ".join(open(os.path.join(C.ROOT, "include", "fplll_hip.h")).read().replace(" * ", " ").split())
    assert "lll_ex / ladder) return FPHIP_UNSUPPORTED" not in hdr
    assert "fphip_gso_lll_ex (precision 53, 106 and 212) and every stage of fphip_gso_lll_ladder carry u" in hdr
    assert "max(d, n) <= 64 only" in hdr
