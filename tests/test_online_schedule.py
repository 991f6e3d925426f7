"""CPU: the release schedule of tsw_plan_mapd_online (csrc/tsw_online.h) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/online_main.cpp, host compiler, no HIP and no device).
Pinned: unsorted and duplicate release times, releases at 0, at max_t and at max_t + 1, m = 0, a NULL release array,
tasks that are never released, hold ranges that hit max_t, max_t = 0. Swept over seeded schedules with a stand-in for
k_plan: the columns of a run are written once and in order, every task with release <= max_t is released once and at
its time, unreleased tasks keep the run alive to max_t. The program exits non-zero on a failed case; a sanitizer report
aborts it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_online_schedule_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "online_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "p2p_distributed_tswap_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "online_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "online schedule ok" in r.stdout
    assert "FAIL" not in r.stdout
