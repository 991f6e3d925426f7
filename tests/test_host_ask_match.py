"""CPU: the host A* request ring's word layout and match test (csrc/tsw_plan.h: host_req_word, host_req_live,
host_reply_match — what refresh_codes and coop_wait use to decide "this reply answers this agent's pair"), as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/host_ask_match_main.cpp, host
compiler, no HIP and no device). Cases: an exact match, a zeroed ring, the same slot after a wrap (ring of 8, ticket
t against t + 8), a ticket outside the window, another pair under the same ticket, a code of 5, the largest ticket
(HOST_RING_MAX_TICKETS) and cells at 2^20 - 1. The program exits non-zero on a failed case; a sanitizer report
aborts it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_ask_match_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "host_ask_match_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "p2p_distributed_tswap_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "host_ask_match_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "host ask match ok" in r.stdout
    assert "FAIL" not in r.stdout
