"""CPU: the LDS placement and kernel-choice rules (csrc/tsw_place.h) as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/host/place_main.cpp, host compiler, no HIP and no device). Pinned: the planner
placement (six flags, k_plan instantiation, LDS bytes) of every parity case that profiles/r16/gpu_tests.txt and
profiles/r17/placement_parent.txt record from an MI355X, all seven instantiations among them; the worker layouts of C3,
wh10k and C5 (1,020 / 1,275 / 2,295 waves); den520d -> k_bfs_blk, 1024x1024 -> k_bfs_big, the 2048x33 grid that does
not fit k_bfs_mg (169,412 B); the 16-byte bitmap padding on 200x130. The last parameter of choose_plan_placement
(agents_on, TSW_AGENTS_LDS) left out gives every recorded placement; the three placements of tests/test_gpu_rules.py (ag,
global, pg) at the fleets and grids of tests/rules_cases.py. Swept over grids from 1x1 to the 2^20-cell and
2048-side limits, 1 .. 65,535 agents, 64 and 160 KiB of LDS, 1 and 256 CUs: a placement fits its budget, mu implies occ
and 16-bit agent ids, every placement has an instantiation; a worker layout fits the dispatch's LDS and keeps the staged
bitmap beside LDS g-scores; a K1 choice fits, a forced kernel that does not reports itself, the default mode always has
a kernel, mg is never chosen in a library without it. The program exits non-zero on a failed case; a sanitizer report
aborts it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_place_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "place_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "p2p_distributed_tswap_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "place_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "place ok" in r.stdout
    assert "FAIL" not in r.stdout
