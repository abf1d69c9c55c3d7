"""Static guards of the fifth-generation walk (enum_walk5_kernel<MU_LDS, DUAL>, enum_walk5.hip: the text of
enum_walk.hip compiled with FPHIP_WALK5 — DESIGN.md section 3), on the compiled enum_walk5.hip:

  * its loops hold wave-uniform branches only; 64 VGPRs with at most 16 bytes of scratch per lane for every
    instantiation, none of it touched by the EXPAND loop;
  * the chain link stays within the third generation's budget (test_isa_walk_link.BUDGET) but for one s_mov_b32: the
    rotation reorders the link, it adds no vector instruction and no branch to it;
  * the rotation: the header of the EXPAND loop asks for nothing (no ds_bpermute, no s_load, no buffer load) — the
    chain-descent block does, behind the column update and BEFORE its count and its DPP move;
  * the no-tie pair path — from the block that reads the sibling's distance off the test (row_newbcast:1 or :2) back to
    the loop header: no double-precision compare, no v_mul_f64 but the two column products, no writelane, four selects
    (x_2 and nd_2 into the level's lane), and the double-precision adds are x_2, the two column updates (DUAL: and
    a_2 = x_2 - c);
  * the tie pair keeps the fourth generation's computation: one block of the loop still holds the direction compare
    against the centre with its select;
  * the descent with three or more children keeps six selects and one writelane;
  * the pair STEP as test_isa_walk4.py pins it.

(The fused add of the issue — the first child's distance by v_fmac_f64 with DPP — was measured and is not in the kernel:
no v_fmac_f64 anywhere in it.)  CPU-only, on the helpers of test_isa_walk.py, test_isa_walk_link.py, test_isa_walk4.py."""
import os
import re
import subprocess

import pytest

import conftest as C
from test_isa_uniform_loops import FLAGS, OPT, _hipcc, _kernel_body
from test_isa_walk import _count, _expand_loop
from test_isa_walk4 import LANE_SELECT, _pair_step
from test_isa_walk_link import BUDGET, _counts, _loop_in_text_order, _paths, _successors

SRC = os.path.join(C.ROOT, "fplll_amd", "csrc", "enum_walk5.hip")
KERNEL = "_ZN5fphip17enum_walk5_kernelILb%dELb%dE"
ANY5 = r"_ZN5fphip17enum_walk5_kernelILb[01]ELb[01]E"
INSTANCES = [(0, 0), (0, 1), (1, 0), (1, 1)]
DPP0 = re.compile(r"v_mov_b64_dpp\b.*\brow_newbcast:0\b")
DPP12 = re.compile(r"v_mov_b64_dpp\b.*\brow_newbcast:[12]\b")
ASKS = ("ds_bpermute", "s_load", "buffer_load", "global_load")

pytestmark = pytest.mark.skipif(_hipcc() is None or not os.path.exists(OPT), reason="needs hipcc and opt")


@pytest.fixture(scope="module")
def artefacts5(tmp_path_factory):
    from fplll_amd import build
    d = tmp_path_factory.mktemp("isa_walk5")
    ll, asm = str(d / "walk5.ll"), str(d / "walk5.s")
    assert "enum_walk5.hip" in build.HIP_SOURCES
    assert build.EXTRA_DEPS["enum_walk5.hip"] == ["enum_walk.hip"]
    per_file = build.PER_FILE_FLAGS["enum_walk5.hip"]
    assert per_file == build.PER_FILE_FLAGS["enum_walk.hip"]
    front = [f for i, f in enumerate(per_file) if f != "-mllvm" and (i == 0 or per_file[i - 1] != "-mllvm")]
    subprocess.check_call([_hipcc()] + FLAGS + front + ["-S", "-emit-llvm", "-o", ll, SRC], stderr=subprocess.DEVNULL)
    subprocess.check_call([_hipcc()] + FLAGS + per_file + ["-S", "-o", asm, SRC], stderr=subprocess.DEVNULL)
    uni = subprocess.run([OPT, "-mtriple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-passes=print<uniformity>",
                          "-disable-output", ll], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, check=True)
    return uni.stderr.decode(), open(asm).read()


def test_walk5_kernels_have_no_loop_with_a_divergent_exit(artefacts5):
    uni, _ = artefacts5
    seen = 0
    for p in uni.split("UniformityInfo for function ")[1:]:
        name = p.split("'")[1]
        if not re.match(ANY5, name):
            continue
        seen += 1
        cycles = [l for l in p.split("\n") if l.strip().startswith("depth=") and len(l.split(")")[-1].split()) >= 2]
        assert not cycles, "%s: loops with a divergent exit: %s" % (name, cycles[:2])
    assert seen == 4


def test_walk5_resources(artefacts5):
    _, asm = artefacts5
    meta = asm[asm.index(".amdgpu_metadata"):]
    seen = 0
    for m in re.finditer(r"\.name:\s+(%s\S+)" % ANY5, meta):
        blk = meta[max(0, meta.rfind("- .agpr_count", 0, m.start())):meta.find("- .agpr_count", m.end())]
        seg = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        assert seg and vg, m.group(1)
        assert int(seg.group(1)) <= 16 and int(vg.group(1)) <= 64, (m.group(1), seg.group(1), vg.group(1))
        seen += 1
    assert seen == 4


def _selects(ins):
    """the selects of a level's lane registers: sel_i32's VOP3 form with the level's bit in an SGPR pair."""
    return sum(bool(re.match(r"v_cndmask_b32_e64\s+\S+\s+\S+\s+\S+\s+s\[", s)) for s in ins)


def _chain_block(members):
    """the chain-descent block: counts its node, hands the first child's distance to the rows, stores nothing."""
    got = [b for b in members if any(DPP0.match(s) for s in b[2]) and any(s.startswith("v_addc_co_u32") for s in b[2])
           and _selects(b[2]) == 0 and _count(b[2])["writelane"] == 0]
    assert len(got) == 1, [b[0] for b in got]
    return got[0]


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_expand_loop_holds_no_scratch_no_exec_write_no_fused_add(artefacts5, mu_lds, dual):
    _, asm = artefacts5
    body = _kernel_body(asm, KERNEL % (mu_lds, dual))
    loop = _expand_loop(body)
    assert loop is not None
    ins = [s for b in loop for s in b[2]]
    c = _count(ins)
    assert c["execs"] == 0 and c["scratch"] == 0, c
    assert not any(s.startswith("v_fmac_f64") for s in body)
    # one count per descent: the chain, the two ends of the pair (tie / no tie) and the descent with siblings
    assert 3 <= sum(s.startswith("v_addc_co_u32") for s in ins) <= 4


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_the_loop_is_rotated(artefacts5, mu_lds, dual):
    _, asm = artefacts5
    header, members = _loop_in_text_order(_kernel_body(asm, KERNEL % (mu_lds, dual)))
    assert header is not None
    assert not any(s.startswith(ASKS) for s in header[2]), header[2]
    assert any(s.startswith("v_rndne_f64") for s in header[2])
    chain = _chain_block(members)
    ins = chain[2]
    first = lambda pre: next(i for i, s in enumerate(ins) if s.startswith(pre))  # noqa: E731
    bp = first("ds_bpermute")
    assert sum(s.startswith("ds_bpermute") for s in ins) == 2
    assert first("v_mul_f64") < bp and first("v_add_f64") < bp  # the child's column first
    assert bp < first("v_addc_co_u32") and bp < first("v_mov_b64_dpp")  # the bookkeeping behind the requests
    assert any(s.startswith("s_load_dwordx4") for s in ins)
    # (the mu row from LDS: the compiler sinks the identical ds_read of every descent into the header, behind the
    #  broadcast's wait — the buffer load of the big launches' instantiations stays with the descent)
    if mu_lds:
        assert sum(s.startswith("ds_read_b64") for s in ins + header[2]) == 1
    else:
        assert any(s.startswith("buffer_load_dwordx2") for s in ins)


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_chain_link_within_the_third_generations_budget(artefacts5, mu_lds, dual):
    _, asm = artefacts5
    header, members = _loop_in_text_order(_kernel_body(asm, KERNEL % (mu_lds, dual)))
    chain = _chain_block(members)
    ci, h = members.index(chain), members.index(header)
    # off the link: every other block that counts a node (the descents with siblings)
    avoid = {i for i, b in enumerate(members) if i != ci and any(s.startswith("v_addc_co_u32") for s in b[2])}
    succ = _successors(members)
    size = lambda p: sum(len(members[i][2]) for i in p)  # noqa: E731
    down = min(_paths(succ, h, ci, avoid), key=size)
    up = min(_paths(succ, ci, h, avoid), key=size)
    link = [members[i] for i in down + up[1:-1]]
    (valu, salu, cbr, br), ins = _counts(link)
    print("chain link <%d, %d>: %d VALU, %d SALU, %d conditional, %d unconditional branches" % (mu_lds, dual, valu, salu, cbr, br))
    # the third generation's budget, and ONE scalar instruction more: the level number lives in two SGPRs across the
    # back edge (the descent asks with the new one, the header's exits read the old), an s_mov_b32 joins them
    want = BUDGET[(mu_lds, dual)]
    assert valu <= want[0] and salu <= want[1] + 1 and cbr <= want[2] and br <= want[3], ((valu, salu, cbr, br), ins)
    assert sum(s.startswith("ds_bpermute") for s in ins) == 2


def _no_tie_pair_paths(members, header):
    """every path from a block that reads the sibling's distance off the test (row_newbcast:1 / :2) to the header."""
    starts = [i for i, b in enumerate(members) if any(DPP12.match(s) for s in b[2])]
    assert len(starts) == 2, [members[i][0] for i in starts]
    succ = _successors(members)
    h = members.index(header)
    out = []
    for s0 in starts:
        ps = _paths(succ, s0, h, set())
        assert ps
        out += [[members[i] for i in p[:-1]] for p in ps]
    return out


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_no_tie_pair_path(artefacts5, mu_lds, dual):
    _, asm = artefacts5
    header, members = _loop_in_text_order(_kernel_body(asm, KERNEL % (mu_lds, dual)))
    paths = _no_tie_pair_paths(members, header)
    assert 2 <= len(paths) <= 4  # two directions, the LDS and the global slot of the push
    for path in paths:
        ins = [s for b in path for s in b[2]]
        assert not any(re.match(r"v_cmpx?_\w+_f64", s) for s in ins), ins
        assert sum(s.startswith("v_mul_f64") for s in ins) == 2, ins  # the two column products
        assert sum(s.startswith("v_add_f64") for s in ins) == (4 if dual else 3), ins  # x_2, S_2, S_1 (DUAL: a_2)
        assert not any(s.startswith(("v_writelane", "v_fma_f64", "v_fmac_f64")) for s in ins), ins
        assert _selects(ins) == 4, ins
        assert sum(bool(DPP12.match(s)) for s in ins) == 1 and sum(bool(DPP0.match(s)) for s in ins) == 1
        assert sum(s.startswith("v_addc_co_u32") for s in ins) == 1
        assert sum(s.startswith("ds_bpermute") for s in ins) == 2  # the next centre, asked for by the descent
        assert any(re.match(r"v_add_f64\s+\S+\s+\S+\s+-?1\.0$", s) for s in ins), ins  # x_2 = x_0 +- 1.0, inline


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_tie_pair_and_wide_descent_keep_their_computation(artefacts5, mu_lds, dual):
    _, asm = artefacts5
    header, members = _loop_in_text_order(_kernel_body(asm, KERNEL % (mu_lds, dual)))
    # the direction of a tie pair: c >= x_0 after the correction, a compare of two VGPR pairs feeding a select of +-1.0
    direction = [b for b in members
                 if any(re.match(r"v_cmp_(le|ge)_f64", s) for s in b[2]) and any(s.startswith("v_cndmask_b32_e32") for s in b[2])
                 and any(s.startswith("v_mul_f64") for s in b[2])]
    assert len(direction) >= 1
    wide = [b for b in members if _count(b[2])["writelane"] == 1]
    assert len(wide) == 1
    assert _selects(wide[0][2]) == 6, wide[0][2]
    half = [s for b in members for s in b[2] if re.match(r"v_cmpx?_\w+_f64\w*\s.*\b0\.5\b", s)]
    assert len(half) == 1  # the tie test once, off the link
    assert not any(re.match(r"v_cmpx?_\w+_f64\w*\s.*\b0\.5\b", s) for s in header[2])


@pytest.mark.parametrize("mu_lds,dual", INSTANCES)
def test_pair_step_pops_and_broadcasts_and_nothing_else(artefacts5, mu_lds, dual):
    """As test_isa_walk4.py pins it: LDS path 2 VALU, 1 ds_read_b64, 2 ds_bpermute, no readlane; global path 3 VALU,
    1 global_load, 2 ds_bpermute, 2 v_readlane with a constant lane."""
    _, asm = artefacts5
    search, step = _pair_step(_kernel_body(asm, KERNEL % (mu_lds, dual)))
    assert step is not None
    lds_blk = [c for c in step if any(s.startswith("ds_read") for s in c[2])]
    glb_blk = [c for c in step if any(s.startswith("global_load") for s in c[2])]
    assert len(lds_blk) == 1 and len(glb_blk) == 1 and lds_blk[0] is not glb_blk[0]
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
