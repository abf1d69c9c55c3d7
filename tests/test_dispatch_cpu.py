"""fplll_amd/csrc/host_common.h — the dispatchers from a run-time width class (columns per lane, 1 .. 4) and from a
precision (53 / 106 / 212 bits) to a kernel instantiation, compiled for the HOST (tests/native/dispatch_host.cpp):
nq = 1, 2, 3, 4 reach 1, 2, 3, 4 and 5 reaches 4, the precisions reach double / DD / QD, each exactly once.  Every
launch site of the host files goes through these two functions."""
import os
import subprocess

import conftest as C


def test_dispatchers_on_the_host(tmp_path):
    exe = str(tmp_path / "dispatch_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(C.ROOT, "tests", "native", "dispatch_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and len(lines) == 11, r.stdout + r.stderr
    assert all(l.startswith("ok ") for l in lines), [l for l in lines if not l.startswith("ok ")]
