"""Compile-time facts of the quadratic-form LLL kernel (fplll_amd/csrc/lll_gram.hip): the object holds all four
width-class instantiations of lll_gram_kernel<NQ> and each stays within the 256 registers per lane a wavefront can
have.  The counts are printed (pytest -s) and recorded in DESIGN.md 4i; no tighter budget is asserted than that.
CPU-only, on the object build() left behind, with the helpers of tests/test_kernel_budgets.py."""
import pytest

import test_kernel_budgets as B

pytestmark = B.pytestmark


def test_lll_gram_kernels_are_all_there_and_fit(tmp_path):
    ks = B._kernels("lll_gram.hip", str(tmp_path))
    for nq in (1, 2, 3, 4):
        (k, (regs, scratch)), = B._pick(ks, r"lll_gram_kernelILi%dEE" % nq).items()
        print("lll_gram_kernel<%d>: %d registers, %d bytes of scratch per lane" % (nq, regs, scratch))
        assert regs <= 256, (k, regs)
        (k, (regs, scratch)), = B._pick(ks, r"gram_update_kernelILi%dEE" % nq).items()
        print("gram_update_kernel<%d>: %d registers, %d bytes of scratch per lane" % (nq, regs, scratch))
        assert regs <= 256, (k, regs)
