"""Static guards of the CHAIN LINK of the third-generation walk (enum_walk_kernel<MU_LDS, DUAL, CHAIN = true>,
enum_walk.hip): the cycle of the EXPAND loop a node with exactly one child takes — loop header,
the 64-lane test, the exits it passes, the chain-descent block, the shared tail, back to the header.  Two thirds of
the nodes of the flagship tree are reached through it.

What the change took out of the link stays out: roundto()'s tie test.  Between the loop header and the ballot's
popcount there is no double-precision compare with 0.5 — the vector test runs around rint(c), the tie is corrected on
the descent with siblings, in a block the link does not pass.

The budgets are the counts of the shipped build.  The parent's link, counted the same way (SALU as test_isa_walk.py
counts it: every s_ instruction but s_nop, s_waitcnt and the branches — the s_load of (r, pruning) included, which makes
the 9 SALU of a count without it 10): 14 VALU, 10 SALU, 5 conditional branches, no unconditional one.  The tie test
was one VALU and one conditional branch of those.  (The scalar-side items measured with it — the special levels as a
mask test, induction variables for the level's bit and row offset, B cleared once per step, the popcount compared
with 4 first: a link of 13 / 7 / 3 / 0 — bought 0.2 % together and are not in the kernel: DESIGN.md section 3.)

CPU-only, on the helpers and the compiled artefacts of test_isa_walk.py."""
import re

import pytest

from test_isa_walk import KERNEL, _blocks, _kernel_body, artefacts, pytestmark  # noqa: F401

INSTANCES = [(0, 0), (0, 1), (1, 0), (1, 1)]
# (VALU, SALU, conditional branches, unconditional branches) of the link: the parent's 14 / 10 / 5 / 0 of the
# buffer-load instantiations less the tie test's VALU and branch.  MU_LDS addresses its packed mu rows by the level
# number: 16 / 16 / 5 / 0 in the parent, less the same two here.
BUDGET = {(0, 0): (13, 10, 4, 0), (0, 1): (13, 10, 4, 0), (1, 0): (15, 16, 4, 0), (1, 1): (15, 16, 4, 0)}
HALF = re.compile(r"v_cmpx?_\w+_f64\w*\s.*\b0\.5\b")


def _loop_in_text_order(body):
    blocks = _blocks(body)
    for b in blocks:
        if "This Inner Loop Header" in b[1] and b[0]:
            members = [c for c in blocks if c is b or re.search(r"in Loop: Header=BB%s\b" % b[0], c[1])]
            ins = [s for c in members for s in c[2]]
            if any(s.startswith("v_rndne_f64") for s in ins) and any(s.startswith("s_bcnt1_i32_b64") for s in ins):
                return b, members
    return None, None


def _successors(members):
    """index -> [(index of the successor, taken through a branch?)] inside the loop."""
    by_name = {c[0]: i for i, c in enumerate(members) if c[0]}
    succ = {}
    for i, c in enumerate(members):
        out = []
        for s in c[2]:
            m = re.match(r"s_c?branch\w*\s+\.LBB(\d+_\d+)", s)
            if m and m.group(1) in by_name:
                out.append((by_name[m.group(1)], True))
        if not (c[2] and c[2][-1].startswith("s_branch")) and i + 1 < len(members):
            out.append((i + 1, False))  # falls through (blocks that leave the loop sit behind it)
        succ[i] = out
    return succ


def _paths(succ, a, b, avoid):
    """every simple path a -> b that stays off `avoid`."""
    out, stack = [], [(a, [a])]
    while stack:
        n, p = stack.pop()
        for t, _ in succ[n]:
            if t == b:
                out.append(p + [b])
            elif t not in p and t not in avoid:
                stack.append((t, p + [t]))
    return out


def _link(body):
    """The blocks of the chain link in the order they run: header -> ... -> chain-descent block -> ... -> header."""
    header, members = _loop_in_text_order(body)
    assert header is not None
    adds = [i for i, c in enumerate(members) if any(s.startswith("v_addc_co_u32") for s in c[2])]
    chain = [i for i in adds if not any(s.startswith("v_writelane") for s in members[i][2])]
    wide = [i for i in adds if i not in chain]
    assert len(chain) == 1 and len(wide) == 1
    succ = _successors(members)
    h = members.index(header)
    size = lambda p: sum(len(members[i][2]) for i in p)  # noqa: E731
    down = min(_paths(succ, h, chain[0], set(wide)), key=size)
    up = min(_paths(succ, chain[0], h, set(wide)), key=size)
    return [members[i] for i in down + up[1:-1]], members


def _counts(link):
    ins = []
    for n, c in enumerate(link):
        nxt = link[(n + 1) % len(link)]
        for s in c[2]:
            # an unconditional branch is paid only where the link takes it: at the end of its block
            if s.startswith("s_branch") and not (nxt[0] and s.endswith(".LBB" + nxt[0])):
                continue
            ins.append(s)
    return (sum(s.startswith("v_") for s in ins),
            sum(s.startswith("s_") and not s.startswith(("s_nop", "s_waitcnt", "s_cbranch", "s_branch")) for s in ins),
            sum(s.startswith("s_cbranch") for s in ins),
            sum(s.startswith("s_branch") for s in ins)), ins


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_no_tie_test_between_the_loop_header_and_the_popcount(artefacts, mu_lds, dual):
    _, asm = artefacts
    link, members = _link(_kernel_body(asm, KERNEL % (mu_lds, dual, 1)))
    seen = False
    for c in link:
        for s in c[2]:
            assert not HALF.match(s), (c[0], s)
            if s.startswith("s_bcnt1_i32_b64"):
                seen = True
                break
        if seen:
            break
    assert seen
    # the test exists — once, in a block of the loop that is no part of the link
    rest = [s for c in members if c not in link for s in c[2]]
    assert sum(bool(HALF.match(s)) for s in rest) == 1
    assert not any(HALF.match(s) for c in link for s in c[2])


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_chain_link_within_its_budgets(artefacts, mu_lds, dual):
    _, asm = artefacts
    link, _ = _link(_kernel_body(asm, KERNEL % (mu_lds, dual, 1)))
    (valu, salu, cbr, br), ins = _counts(link)
    want = BUDGET[(mu_lds, dual)]
    assert valu <= want[0] and salu <= want[1] and cbr <= want[2] and br <= want[3], ((valu, salu, cbr, br), ins)
    # below the parent's 14 / 10 / 5 / 0 by what the kept item removes (the buffer-load instantiations)
    if not mu_lds:
        assert valu <= 14 - 1 and salu <= 10 and cbr <= 5 - 1 and br == 0
