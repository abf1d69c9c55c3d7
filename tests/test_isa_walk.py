"""Static guards of the walk kernels' performance contracts (enum_walk.hip — one kernel text for both generations,
enum_walk_kernel<MU_LDS, DUAL, CHAIN> — DESIGN.md section 3).

Second generation (CHAIN = false): its two hot loops — the EXPAND chain (all children of a node in one 64-lane test)
and the STEP loop (the next sibling by index) — hold wave-uniform branches only, no scratch traffic and no
register-copy storms, stay within the static instruction budgets the per-node PMC figures correspond to
(profiles/r06_enum_walk2_pmc_*.txt: 26 VALU + 20 SALU + 8 branch + 5.5 LDS per node), and the kernel keeps 8 waves per
SIMD.  The LDS unit is shared by the four SIMDs of a CU: every ds_bpermute in these loops was measured to cost
throughput, so their number is pinned as well.

Third generation (CHAIN = true): its EXPAND loop holds wave-uniform branches only, no scratch traffic and no exec
writes; a chain descent (a node with exactly one child — two thirds of the nodes of the flagship tree) stores nothing:
no ds_write, no lane-register select, within a small VALU budget; the next sibling is found by one scalar search
(s_ff1) instead of a climbing loop; and the kernel keeps 8 waves per SIMD.

CPU-only: hipcc emits the optimised IR / ISA for gfx950 once for the module, `opt` prints the uniformity analysis."""
import os
import re
import subprocess

import pytest

import conftest as C
from test_isa_uniform_loops import FLAGS, OPT, _hipcc, _innermost_loops, _kernel_body

SRC = os.path.join(C.ROOT, "fplll_amd", "csrc", "enum_walk.hip")
# <MU_LDS = false, DUAL = false>: the big launches, per generation (the third template argument is CHAIN)
KERNEL = "_ZN5fphip16enum_walk_kernelILb%dELb%dELb%dE"
WALK2 = KERNEL % (0, 0, 0)
WALK3 = KERNEL % (0, 0, 1)
ANY2 = r"_ZN5fphip16enum_walk_kernelILb[01]ELb[01]ELb0E"  # every instantiation of a generation
ANY3 = r"_ZN5fphip16enum_walk_kernelILb[01]ELb[01]ELb1E"

pytestmark = pytest.mark.skipif(_hipcc() is None or not os.path.exists(OPT), reason="needs hipcc and opt")


@pytest.fixture(scope="module")
def artefacts(tmp_path_factory):
    from fplll_amd import build
    d = tmp_path_factory.mktemp("isa_walk")
    ll, asm = str(d / "walk.ll"), str(d / "walk.s")
    assert "enum_walk.hip" in build.HIP_SOURCES
    assert "enum_walk3.hip" not in build.HIP_SOURCES  # (folded into enum_walk.hip)
    per_file = build.PER_FILE_FLAGS["enum_walk.hip"]
    assert "-structurizecfg-skip-uniform-regions=1" in per_file and "-disable-lifetime-markers" in per_file
    front = [f for i, f in enumerate(per_file) if f != "-mllvm" and (i == 0 or per_file[i - 1] != "-mllvm")]
    subprocess.check_call([_hipcc()] + FLAGS + front + ["-S", "-emit-llvm", "-o", ll, SRC], stderr=subprocess.DEVNULL)
    subprocess.check_call([_hipcc()] + FLAGS + per_file + ["-S", "-o", asm, SRC], stderr=subprocess.DEVNULL)
    uni = subprocess.run([OPT, "-mtriple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-passes=print<uniformity>",
                          "-disable-output", ll], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, check=True)
    return uni.stderr.decode(), open(asm).read()


def _no_loop_with_a_divergent_exit(uni, generation):
    seen = 0
    for p in uni.split("UniformityInfo for function ")[1:]:
        name = p.split("'")[1]
        if not re.match(generation, name):
            continue
        seen += 1
        cycles = [l for l in p.split("\n") if l.strip().startswith("depth=") and len(l.split(")")[-1].split()) >= 2]
        assert not cycles, "%s: loops with a divergent exit: %s" % (name, cycles[:2])
    assert seen == 4


def _resources(asm, generation):
    """64 VGPRs (8 waves per SIMD) with at most 16 bytes of scratch per lane, for all four instantiations."""
    meta = asm[asm.index(".amdgpu_metadata"):]
    seen = 0
    for m in re.finditer(r"\.name:\s+(%s\S+)" % generation, meta):
        blk = meta[max(0, meta.rfind("- .agpr_count", 0, m.start())):meta.find("- .agpr_count", m.end())]
        seg = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        assert seg and vg, m.group(1)
        assert int(seg.group(1)) <= 16 and int(vg.group(1)) <= 64, (m.group(1), seg.group(1), vg.group(1))
        seen += 1
    assert seen == 4


def _blocks(body):
    """(name, loop-comment, instructions) of every basic block of a kernel body."""
    out, cur = [], None
    for l in body:
        m = re.match(r"^\.LBB(\d+_\d+):(.*)$", l)
        if m or l.startswith("; %bb."):
            cur = [m.group(1) if m else None, m.group(2) if m else l, []]
            out.append(cur)
        elif cur is not None:
            s = l.strip()
            if s.startswith(";") and "Loop" in s:
                cur[1] += " " + s
            elif s and not s.startswith(";"):
                cur[2].append(s)
    return out


def _expand_loop(body):
    """The blocks of the innermost loop that holds the vector roundto and the ballot's popcount."""
    blocks = _blocks(body)
    for b in blocks:
        if "This Inner Loop Header" in b[1] and b[0]:
            members = [b] + [c for c in blocks if re.search(r"in Loop: Header=BB%s\b" % b[0], c[1])]
            ins = [s for c in members for s in c[2]]
            if any(s.startswith("v_rndne_f64") for s in ins) and any(s.startswith("s_bcnt1_i32_b64") for s in ins):
                return members
    return None


def _count(seg):
    return dict(valu=sum(s.startswith("v_") for s in seg),
                lds=sum(s.startswith("ds_") for s in seg),
                ds_write=sum(s.startswith("ds_write") for s in seg),
                scratch=sum(s.startswith("scratch_") for s in seg),
                execs=sum(bool(re.match(r"s_\w+\s+exec\b", s)) or "saveexec" in s for s in seg),
                cndmask=sum(s.startswith("v_cndmask") for s in seg),
                writelane=sum(s.startswith("v_writelane") for s in seg))


# ---- second generation

def test_walk2_kernels_have_no_loop_with_a_divergent_exit(artefacts):
    uni, _ = artefacts
    _no_loop_with_a_divergent_exit(uni, ANY2)


def test_walk2_hot_loops_within_their_budgets(artefacts):
    _, asm = artefacts
    body = _kernel_body(asm, WALK2)
    found = {}
    for seg in _innermost_loops(body):
        # the EXPAND chain is the innermost loop with the vector roundto; the STEP loop is the readlane-and-compare
        # loop right behind it (its body is the code that follows the loop)
        if any(s.startswith("v_rndne_f64") for s in seg) and any(s.startswith("s_bcnt1_i32_b64") for s in seg):
            key = "expand"
        elif len(seg) <= 12 and any(s.startswith("v_readlane_b32") for s in seg) and any("s_bfe_u32" in s for s in seg):
            key = "step_check"
        else:
            continue
        found[key] = dict(valu=sum(s.startswith("v_") for s in seg),
                          salu=sum(s.startswith("s_") and not s.startswith(("s_nop", "s_waitcnt", "s_cbranch", "s_branch"))
                                   for s in seg),
                          lds=sum(s.startswith("ds_") for s in seg),
                          mov=sum(s.startswith("v_mov") for s in seg),
                          scratch=sum(s.startswith("scratch_") for s in seg),
                          execs=sum(bool(re.match(r"s_\w+\s+exec\b", s)) or "saveexec" in s for s in seg),
                          rl=sum(s.startswith(("v_readlane", "v_readfirstlane")) for s in seg))
    assert set(found) == {"expand", "step_check"}, found
    e = found["expand"]
    # (static counts of ALL blocks of the loop: the tie-rounding and global-stack blocks included)
    # (one v_readlane: the reload of a spilled scalar in the global-stack block)
    assert e["execs"] == 0 and e["scratch"] == 0 and e["rl"] <= 1, e
    assert e["valu"] <= 42 and e["salu"] <= 24 and e["mov"] <= 4 and e["lds"] <= 6, e
    s = found["step_check"]
    assert s["execs"] == 0 and s["scratch"] == 0 and s["valu"] <= 2 and s["salu"] <= 6 and s["lds"] == 0, s
    m = re.search(re.escape(WALK2) + r"[^\n]*\n(?:.*\n)*?\s*\.vgpr_count:\s+(\d+)", asm[asm.index(".amdgpu_metadata"):])
    assert m and int(m.group(1)) <= 64, m and m.group(1)


def test_walk2_scratch_is_confined_to_the_slow_paths(artefacts):
    """64 VGPRs (8 waves per SIMD) with at most 16 bytes of scratch per lane, none of it touched by the hot loops."""
    _, asm = artefacts
    _resources(asm, ANY2)


# ---- third generation

def test_walk3_kernels_have_no_loop_with_a_divergent_exit(artefacts):
    uni, _ = artefacts
    _no_loop_with_a_divergent_exit(uni, ANY3)


def test_walk3_chain_descent_stores_nothing(artefacts):
    """The chain-descent block — the block of the EXPAND loop that counts the child (v_addc) without a writelane —
    holds the child's distance (two bpermutes), the column update and the count: at most 6 VALU, no ds_write, no
    select.  The descent with siblings keeps the push and the lane-register writes."""
    _, asm = artefacts
    loop = _expand_loop(_kernel_body(asm, WALK3))
    assert loop is not None
    ins = [s for b in loop for s in b[2]]
    whole = _count(ins)
    assert whole["execs"] == 0 and whole["scratch"] == 0, whole
    adds = [b for b in loop if any(s.startswith("v_addc_co_u32") for s in b[2])]
    chain = [b for b in adds if not any(s.startswith("v_writelane") for s in b[2])]
    wide = [b for b in adds if any(s.startswith("v_writelane") for s in b[2])]
    assert len(chain) == 1 and len(wide) == 1, [b[0] for b in adds]
    c = _count(chain[0][2])
    assert c["valu"] <= 6 and c["ds_write"] == 0 and c["cndmask"] == 0 and c["lds"] <= 2, c
    w = _count(wide[0][2])
    assert w["writelane"] == 1 and w["cndmask"] == 6, w


def test_walk3_step_is_one_scalar_search(artefacts):
    """STEP finds the level of the next sibling with s_ff1 on the mask P; no innermost loop of the kernel climbs
    level by level (the readlane-and-compare loop of the second generation)."""
    _, asm = artefacts
    body = _kernel_body(asm, WALK3)
    assert any(l.strip().startswith("s_ff1_i32_b64") for l in body)
    blocks = _blocks(body)
    for b in blocks:
        if "This Inner Loop Header" in b[1] and b[0]:
            ins = [s for c in [b] + [c for c in blocks if re.search(r"in Loop: Header=BB%s\b" % b[0], c[1])]
                   for s in c[2]]
            climb = len(ins) <= 12 and any(s.startswith("v_readlane_b32") for s in ins) and \
                any("s_bfe_u32" in s for s in ins)
            assert not climb, ins


def test_walk3_resources(artefacts):
    """64 VGPRs (8 waves per SIMD) with at most 16 bytes of scratch per lane, for all four instantiations."""
    _, asm = artefacts
    _resources(asm, ANY3)
