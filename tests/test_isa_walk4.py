"""Static guards of the fourth-generation walk (enum_walk4_kernel<MU_LDS, DUAL>, enum_walk4.hip: the text of
enum_walk.hip compiled with FPHIP_WALK4 — DESIGN.md section 3), on the compiled enum_walk4.hip:

  * its loops hold wave-uniform branches only; 64 VGPRs with at most 16 bytes of scratch per lane for every
    instantiation, none of it touched by the EXPAND loop;
  * the chain link — header, the 64-lane test, the exits it passes, the chain-descent block, the shared tail — stays
    within the third generation's budget (test_isa_walk_link.py): the pair format costs the link nothing.  (Counts per
    run — no v_addc in the EXPAND loop, one per run of a bit range — were built, measured and not kept: DESIGN.md
    section 3.  Every descent block and every step counts its node with one v_addc, as in the third generation.);
  * the pair descent keeps four selects (x_2 and nd_2 into the level's lane) and no writelane; the descent with three or
    more children keeps the third generation's six selects and one writelane;
  * the pair STEP: the level search, then two ds_bpermute (the distance) and ONE read of the column on either path (the
    LDS slot; or the global slot, in a block of its own) — no buffer load of a mu row, no double-precision operation, no
    readlane of the sibling state (none at all on the LDS path; the global path reloads the spilled pointer to the
    global stack from two constant lanes, as the third generation's does).

The budgets are the counts of the shipped build.  CPU-only, on the helpers of test_isa_walk.py / test_isa_walk_link.py."""
import os
import re
import subprocess

import pytest

import conftest as C
from test_isa_uniform_loops import FLAGS, OPT, _hipcc, _kernel_body
from test_isa_walk import _blocks, _count, _expand_loop
from test_isa_walk_link import _counts, _loop_in_text_order, _paths, _successors

SRC = os.path.join(C.ROOT, "fplll_amd", "csrc", "enum_walk4.hip")
KERNEL = "_ZN5fphip17enum_walk4_kernelILb%dELb%dE"
ANY4 = r"_ZN5fphip17enum_walk4_kernelILb[01]ELb[01]E"
INSTANCES = [(0, 0), (0, 1), (1, 0), (1, 1)]
# (VALU, SALU, conditional, unconditional branches) of the chain link: test_isa_walk_link.BUDGET
LINK = {(0, 0): (13, 10, 4, 0), (0, 1): (13, 10, 4, 0), (1, 0): (15, 16, 4, 0), (1, 1): (15, 16, 4, 0)}
DPP = re.compile(r"v_mov_b(64|32)_dpp\b.*\brow_newbcast:0\b")

pytestmark = pytest.mark.skipif(_hipcc() is None or not os.path.exists(OPT), reason="needs hipcc and opt")


@pytest.fixture(scope="module")
def artefacts4(tmp_path_factory):
    from fplll_amd import build
    d = tmp_path_factory.mktemp("isa_walk4")
    ll, asm = str(d / "walk4.ll"), str(d / "walk4.s")
    assert "enum_walk4.hip" in build.HIP_SOURCES
    assert build.EXTRA_DEPS["enum_walk4.hip"] == ["enum_walk.hip"]
    per_file = build.PER_FILE_FLAGS["enum_walk4.hip"]
    assert per_file == build.PER_FILE_FLAGS["enum_walk.hip"]
    front = [f for i, f in enumerate(per_file) if f != "-mllvm" and (i == 0 or per_file[i - 1] != "-mllvm")]
    subprocess.check_call([_hipcc()] + FLAGS + front + ["-S", "-emit-llvm", "-o", ll, SRC], stderr=subprocess.DEVNULL)
    subprocess.check_call([_hipcc()] + FLAGS + per_file + ["-S", "-o", asm, SRC], stderr=subprocess.DEVNULL)
    uni = subprocess.run([OPT, "-mtriple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-passes=print<uniformity>",
                          "-disable-output", ll], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, check=True)
    return uni.stderr.decode(), open(asm).read()


def test_walk4_kernels_have_no_loop_with_a_divergent_exit(artefacts4):
    uni, _ = artefacts4
    seen = 0
    for p in uni.split("UniformityInfo for function ")[1:]:
        name = p.split("'")[1]
        if not re.match(ANY4, name):
            continue
        seen += 1
        cycles = [l for l in p.split("\n") if l.strip().startswith("depth=") and len(l.split(")")[-1].split()) >= 2]
        assert not cycles, "%s: loops with a divergent exit: %s" % (name, cycles[:2])
    assert seen == 4


def test_walk4_resources(artefacts4):
    _, asm = artefacts4
    meta = asm[asm.index(".amdgpu_metadata"):]
    seen = 0
    for m in re.finditer(r"\.name:\s+(%s\S+)" % ANY4, meta):
        blk = meta[max(0, meta.rfind("- .agpr_count", 0, m.start())):meta.find("- .agpr_count", m.end())]
        seg = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        assert seg and vg, m.group(1)
        assert int(seg.group(1)) <= 16 and int(vg.group(1)) <= 64, (m.group(1), seg.group(1), vg.group(1))
        seen += 1
    assert seen == 4


def _descents(loop):
    """(chain, pair, wide): the blocks of the EXPAND loop that hand the first child's distance to the rows (the DPP
    move), told apart by what they store: nothing / two lane doubles / three and the state word."""
    dpp = [b for b in loop if any(DPP.match(s) for s in b[2])]
    chain = [b for b in dpp if _count(b[2])["cndmask"] == 0]
    wide = [b for b in dpp if _count(b[2])["writelane"] == 1]
    pair = [b for b in dpp if b not in chain and b not in wide]
    assert len(chain) == 1 and len(pair) == 1 and len(wide) == 1, [b[0] for b in dpp]
    return chain[0], pair[0], wide[0]


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_expand_loop_descents(artefacts4, mu_lds, dual):
    _, asm = artefacts4
    loop = _expand_loop(_kernel_body(asm, KERNEL % (mu_lds, dual)))
    assert loop is not None
    ins = [s for b in loop for s in b[2]]
    c = _count(ins)
    assert c["execs"] == 0 and c["scratch"] == 0, c
    chain, pair, wide = _descents(loop)
    # one count per descent block, nowhere else in the loop
    assert [sum(s.startswith("v_addc_co_u32") for s in b[2]) for b in (chain, pair, wide)] == [1, 1, 1]
    assert sum(s.startswith("v_addc_co_u32") for s in ins) == 3
    cc, pc, wc = _count(chain[2]), _count(pair[2]), _count(wide[2])
    assert cc["valu"] <= 2 and cc["lds"] == 0, cc  # (count and move; the column update sits in the shared tail)
    assert pc["cndmask"] == 4 and pc["writelane"] == 0, pc
    assert wc["cndmask"] == 6 and wc["writelane"] == 1, wc


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_chain_link_within_the_third_generations_budget(artefacts4, mu_lds, dual):
    _, asm = artefacts4
    header, members = _loop_in_text_order(_kernel_body(asm, KERNEL % (mu_lds, dual)))
    assert header is not None
    chain, pair, wide = _descents(members)
    ci = members.index(chain)
    avoid = {members.index(pair), members.index(wide)}
    succ = _successors(members)
    h = members.index(header)
    size = lambda p: sum(len(members[i][2]) for i in p)  # noqa: E731
    down = min(_paths(succ, h, ci, avoid), key=size)
    up = min(_paths(succ, ci, h, avoid), key=size)
    link = [members[i] for i in down + up[1:-1]]
    (valu, salu, cbr, br), ins = _counts(link)
    want = LINK[(mu_lds, dual)]
    assert valu <= want[0] and salu <= want[1] and cbr <= want[2] and br <= want[3], ((valu, salu, cbr, br), ins)


def _pair_step(body):
    """(search block, blocks of the pair STEP): from the level search (s_ff1 on P, the test of Q) every block of the
    hot cycle reached through the branch the search does NOT take (that one is the third generation's STEP), down to
    the header of the cycle — the refresh exit leaves the cycle, the EXPAND chain is a loop of its own."""
    blocks = _blocks(body)
    index = {b[0]: i for i, b in enumerate(blocks) if b[0]}
    for i, b in enumerate(blocks):
        m = re.search(r"in Loop: Header=BB(\d+_\d+)\b", b[1])
        if not m or not any(s.startswith("s_ff1_i32_b64") for s in b[2]):
            continue
        inside = re.compile(r"in Loop: Header=BB%s\b" % m.group(1))
        seen, todo = [], [i + 1]
        while todo:
            j = todo.pop()
            if j in seen or j >= len(blocks) or not inside.search(blocks[j][1]):
                continue
            seen.append(j)
            ins = blocks[j][2]
            for s in ins:
                t = re.match(r"s_c?branch\w*\s+\.LBB(\d+_\d+)", s)
                if t and t.group(1) in index:
                    todo.append(index[t.group(1)])
            if not (ins and ins[-1].startswith("s_branch")):
                todo.append(j + 1)
        step = [blocks[j] for j in sorted(seen)]
        if any(s.startswith("ds_bpermute") for c in step for s in c[2]):
            return b, step
    return None, None


LANE_SELECT = re.compile(r"v_readlane_b32\s+\S+,\s*\S+,\s*(s\d+|m0|vcc_lo|vcc_hi)\b")  # a lane chosen at run time


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_pair_step_pops_and_broadcasts_and_nothing_else(artefacts4, mu_lds, dual):
    """The two paths of the pair STEP are counted one by one: the pop from the LDS slot, and the pop from a global slot
    (a block of its own that the other path does not run).  Shipped build, all four instantiations: LDS path 2 VALU
    (slot address, count), 1 ds_read_b64, 2 ds_bpermute, no readlane at all; global path 3 VALU (lane clamp, address,
    count), 1 global_load, 2 ds_bpermute and exactly 2 v_readlane with a CONSTANT lane — the reload of the spilled
    pointer to the global stack, the same reload the third generation's global pop makes."""
    _, asm = artefacts4
    search, step = _pair_step(_kernel_body(asm, KERNEL % (mu_lds, dual)))
    assert step is not None
    lds_blk = [c for c in step if any(s.startswith("ds_read") for s in c[2])]
    glb_blk = [c for c in step if any(s.startswith("global_load") for s in c[2])]
    assert len(lds_blk) == 1 and len(glb_blk) == 1 and lds_blk[0] is not glb_blk[0]
    # the level search reads no lane of the sibling state
    assert not any(s.startswith("v_readlane") for s in search[2]), search[2]
    for name, other, n_valu, n_rl in (("lds", glb_blk[0], 2, 0), ("global", lds_blk[0], 3, 2)):
        ins = [s for c in step if c is not other for s in c[2]]
        reads = [s for s in ins if s.startswith(("ds_read", "global_load", "buffer_load", "s_load", "s_buffer_load",
                                                 "scratch_load"))]
        assert len(reads) == 1 and reads[0].startswith("ds_read_b64" if name == "lds" else "global_load_dwordx2"), reads
        assert sum(s.startswith("ds_bpermute") for s in ins) == 2, (name, ins)
        assert not any(s.startswith(("v_mul_f64", "v_fma_f64", "v_fmac_f64", "v_add_f64", "v_writelane", "v_cndmask",
                                     "scratch_")) for s in ins), (name, ins)
        assert not any(LANE_SELECT.match(s) for s in ins), (name, ins)
        assert sum(s.startswith("v_readlane") for s in ins) == n_rl, (name, ins)
        assert sum(s.startswith("v_") and not s.startswith("v_readlane") for s in ins) <= n_valu, (name, ins)
        assert sum(s.startswith("v_addc_co_u32") for s in ins) == 1, (name, ins)
