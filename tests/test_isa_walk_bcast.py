"""Static guards of the EXPAND loop of enum_walk_kernel<false, false, true> since the first child's distance is a row
broadcast of the vector test's own result (DPP row_newbcast:0 of lane 0's dist_j) and the candidates are a1 + z_j: the
vector instructions that change took out of every node stay out.

The budgets are the counts of the shipped build: 39 VALU in all blocks of the loop (the tie-rounding and global-stack
blocks included; 43 before the change), 10 double-precision multiplies / adds (14 before).  A chain link — loop header,
vector test, chain-descent block, shared tail — issues 14 VALU (17 before).

CPU-only, like test_isa_walk.py, whose helpers and compiled artefacts these tests use."""
import os
import re

import pytest

from test_isa_uniform_loops import OPT, _kernel_body
from test_isa_walk import WALK2, WALK3, _count, _expand_loop, _hipcc, artefacts  # noqa: F401 (artefacts: a fixture)

pytestmark = pytest.mark.skipif(_hipcc() is None or not os.path.exists(OPT), reason="needs hipcc and opt")

DPP = re.compile(r"v_mov_b(64|32)_dpp\b.*\brow_newbcast:0\b")
F64 = re.compile(r"v_(mul|add|fma|fmac)_f64\b")


def _loop(asm, kernel):
    loop = _expand_loop(_kernel_body(asm, kernel))
    assert loop is not None
    return loop


def test_expand_loop_vector_budgets(artefacts):
    _, asm = artefacts
    ins = [s for b in _loop(asm, WALK3) for s in b[2]]
    c = _count(ins)
    f64 = sum(bool(F64.match(s)) for s in ins)
    assert c["valu"] <= 39 and f64 <= 10, (c, f64)
    assert c["execs"] == 0 and c["scratch"] == 0, c


def test_first_childs_distance_is_a_row_broadcast(artefacts):
    """Every descent takes the child's distance through ONE DPP move with row_newbcast:0: either in the tail the
    chain-descent block and the descent with siblings share, or once in each of the two; and the chain-descent block
    still touches neither the LDS crossbar nor LDS memory."""
    _, asm = artefacts
    loop = _loop(asm, WALK3)
    adds = [b for b in loop if any(s.startswith("v_addc_co_u32") for s in b[2])]
    assert len(adds) == 2
    n_dpp = sum(bool(DPP.match(s)) for b in loop for s in b[2])
    in_adds = [sum(bool(DPP.match(s)) for s in b[2]) for b in adds]
    assert (n_dpp == 1 and in_adds == [0, 0]) or (n_dpp == 2 and in_adds == [1, 1]), (n_dpp, in_adds)
    # (one 64-bit move, or the compiler's pair of 32-bit ones — never more)
    assert sum("_dpp" in s for b in loop for s in b[2]) <= 2 * n_dpp
    chain = [b for b in adds if not any(s.startswith("v_writelane") for s in b[2])]
    assert len(chain) == 1
    c = _count(chain[0][2])
    assert c["lds"] == 0 and c["cndmask"] == 0 and c["valu"] <= 6, c
    # the distance is no longer recomputed behind the test: no double-precision multiply feeds an add in the
    # descent blocks except the column update's (one multiply, one add — in the shared tail or in each block)
    for b in adds:
        assert sum(bool(F64.match(s)) for s in b[2]) <= 2, b[2]


def test_a_dpp_read_keeps_its_wait_states(artefacts):
    """Two wait states between a VALU write of a register and its DPP read: the asm statement carries its own s_nop 1
    (the compiler cannot see into it), so the instruction in front of every broadcast is that s_nop — in both
    generations."""
    _, asm = artefacts
    for kernel in (WALK2, WALK3):
        seen = 0
        for b in _loop(asm, kernel):
            for i, s in enumerate(b[2]):
                if DPP.match(s):
                    seen += 1
                    assert i > 0 and re.match(r"s_nop\s+[1-9]", b[2][i - 1]), b[2][max(0, i - 2):i + 1]
        assert seen >= 1, kernel


def test_second_generation_takes_the_same_move(artefacts):
    """The second generation's descent used two ds_bpermute for the first child's distance; it takes the row broadcast
    now: the crossbar carries the centre only."""
    _, asm = artefacts
    ins = [s for b in _loop(asm, WALK2) for s in b[2]]
    assert sum(bool(DPP.match(s)) for s in ins) == 1
    assert sum(s.startswith("ds_bpermute") for s in ins) == 2
