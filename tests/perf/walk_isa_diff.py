"""Maintainer's tool: are the eight walk kernels of the working tree's enum_walk.hip the machine code of a parent
commit's?  A refactor of the walk must answer yes; identical instruction streams are a better proof of unchanged
behaviour and speed than any benchmark.  CPU-only (hipcc cross-compiles for gfx950).

  python tests/perf/walk_isa_diff.py [--parent REV] [--show N]

Both sides are compiled with the flags of fplll_amd/build.py (HIPCC_FLAGS + the per-file flags, --cuda-device-only
-S).  The parent's sources come from `git archive REV`; a parent that still has enum_walk3.hip contributes its
enum_chain_kernel<M, D> as the partner of enum_walk_kernel<M, D, true>, and its enum_walk_kernel<M, D> is the partner
of enum_walk_kernel<M, D, false>.  Per kernel: the lines between its label and its s_endpgm without comments and
directives, the kernel's own mangled name and the function index of local labels (.LBB<n>_<m>) rewritten, and the
resource fields of its .amdgpu_metadata entry.  One result line per kernel; exit status 1 if any differs."""
import argparse
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fplll_amd import build  # noqa: E402

META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".sgpr_spill_count", ".vgpr_spill_count")
SYM = re.compile(r"_ZN5fphip\d+enum_(walk|chain)_kernelILb([01])ELb([01])E(?:Lb([01])E)?\w*")


def _key(m):
    """(MU_LDS, DUAL, CHAIN) of a mangled walk kernel name of either vintage."""
    chain = m.group(1) == "chain" or m.group(4) == "1"
    return (m.group(2) == "1", m.group(3) == "1", chain)


def _asm(csrc, name, out):
    subprocess.check_call([build.hipcc()] + build.HIPCC_FLAGS + build.PER_FILE_FLAGS["enum_walk.hip"] +
                          ["--cuda-device-only", "-S", "-o", out, os.path.join(csrc, name)], stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernels(asm):
    """{(MU_LDS, DUAL, CHAIN): (normalised instruction stream, metadata fields)} of one assembly file."""
    lines, out = asm.split("\n"), {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN5fphip\w+):", l)
        if not m or not SYM.fullmatch(m.group(1)):
            continue
        end = next(j for j in range(i, len(lines)) if "s_endpgm" in lines[j])
        body = []
        for s in lines[i + 1:end + 1]:
            s = s.split(";")[0].rstrip()
            if not s.strip() or (s.strip().startswith(".") and not s.strip().startswith(".LBB")):
                continue
            s = SYM.sub("KERNEL", s)
            s = re.sub(r"__hip_cuid_\w+", "CUID", s)
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
        out[_key(SYM.fullmatch(m.group(1)))] = [body, None]
    meta = asm[asm.index(".amdgpu_metadata"):]
    for m in re.finditer(r"\.name:\s+(_ZN5fphip\w+)", meta):
        k = SYM.fullmatch(m.group(1))
        if not k:
            continue
        blk = meta[max(0, meta.rfind("- .agpr_count", 0, m.start())):meta.find("- .agpr_count", m.end())]
        out[_key(k)][1] = {f: re.search(re.escape(f) + r":\s+(\d+)", blk).group(1) for f in META}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--show", type=int, default=40, help="lines of diff to print per differing kernel")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.check_output(["git", "archive", a.parent, "fplll_amd/csrc"], cwd=ROOT)
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        pc = os.path.join(tmp, "fplll_amd", "csrc")
        old = {}
        for name in ("enum_walk.hip", "enum_walk3.hip"):
            if os.path.exists(os.path.join(pc, name)):
                old.update(_kernels(_asm(pc, name, os.path.join(tmp, "parent_" + name + ".s"))))
        new = _kernels(_asm(os.path.join(ROOT, "fplll_amd", "csrc"), "enum_walk.hip", os.path.join(tmp, "tree.s")))
    bad = set(old) ^ set(new)
    for k in sorted(set(old) & set(new)):
        same = old[k][0] == new[k][0]
        msame = old[k][1] == new[k][1]
        print("enum_walk_kernel<MU_LDS=%d, DUAL=%d, CHAIN=%d>: %5d lines %s; metadata %s (vgpr %s, sgpr %s, scratch %s)"
              % (k + (len(new[k][0]), "identical" if same else "DIFFER", "identical" if msame else "DIFFER",
                      new[k][1][".vgpr_count"], new[k][1][".sgpr_count"], new[k][1][".private_segment_fixed_size"])))
        if not same:
            d = list(difflib.unified_diff(old[k][0], new[k][0], "parent", "tree", lineterm="", n=2))
            print("\n".join(d[:a.show]))
            print("(%d diff lines in all)" % len(d))
        if not msame:
            print("  parent", old[k][1], "\n  tree  ", new[k][1])
        if not (same and msame):
            bad.add(k)
    for k in sorted(set(old) ^ set(new)):
        print("kernel %s is in %s only" % (k, "the parent" if k in old else "the tree"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
