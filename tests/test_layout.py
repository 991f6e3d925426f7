"""CPU: the scratch-block layouts of the host runtime (csrc/tsw_layout.h) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/layout_main.cpp, host compiler, no HIP and no device: the
header includes nothing of HIP, so no HIP include directory is asked for). For each of the eleven blocks (the count
pass, the apply and MAPD state, a tick's decisions, tsw_decide's block, tsw_fleet_apply's inputs, the run and MAPD
records, the audit's outputs, the timeline, a space-time batch), swept over n in {1, 2, 63, 64, 65, 1023, 1024, 1025},
m in {0, 1, 2, 3, 1024, 1025}, T in {1, 2, 3, 1024}, list totals {0, 1, n, 7 n + 3}, grids of {1, 64, 65, 40000} cells,
batches of {1, 2, 4097}, extra words {0, 1}, the optional parts on and off, and the kernel headers' counts at the
library's values and at others: the total is the closed-form sum the call site used to carry, the parts are in order,
disjoint and inside the total, 64-bit parts start on even words, the parts that one memset or copy covers are adjacent,
and a malloc of exactly `total` words takes a write to both ends of every part. The program exits non-zero on a
mismatch; a sanitizer report aborts it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "layout_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "p2p_distributed_tswap_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "layout_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "layout ok" in r.stdout
    assert "FAIL" not in r.stdout
