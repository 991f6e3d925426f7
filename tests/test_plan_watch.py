"""CPU: what the plan dispatch loop shares with the planner by convention (csrc/tsw_plan.h), as a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/plan_watch_main.cpp, host compiler, no HIP and no
device, a fake clock). The watchdog rule (PlanWatchdog): an advancing heartbeat never fires; a still one fires past
watchdog_ms, not at it, once only; a heartbeat that moves afterwards does not fire again; an abort word already set
never fires; watchdog_ms of 1 and 0xFFFFFFFF; a fresh object is armed again. The error table: every bit alone and the
order ERR_ABORT, ERR_BAD_PICKUP, ERR_BAD_DELIVERY, ERR_NO_TABLE (TSW_EINVAL), the rest (TSW_EOVERFLOW). The slot
enums: no two hflags names share a word, room for 16 waves, every sec_ticks name below 64 and the s_tick names below
48. The program exits non-zero on a failed case; a sanitizer report aborts it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_watch_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "plan_watch_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "p2p_distributed_tswap_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "plan_watch_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "plan watch ok" in r.stdout
    assert "FAIL" not in r.stdout
