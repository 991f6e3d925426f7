"""CPU: the host A* translation unit under AddressSanitizer + UndefinedBehaviorSanitizer, as a
stand-alone program (tests/host/host_astar_main.cpp + csrc/tsw_host_astar.cpp, host compiler, no HIP and
no device). The program checks every hop against a BFS and exits non-zero on a mismatch; a sanitizer
report aborts it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_astar_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "host_astar_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "host_astar_main.cpp"),
                           os.path.join(ROOT, "p2p_distributed_tswap_amd", "csrc", "tsw_host_astar.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "host A* sanitizer run ok" in r.stdout
