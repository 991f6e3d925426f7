"""CPU: the owning buffer types of the host runtime (csrc/tsw_buf.h) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/host/devbuf_main.cpp, host compiler, no HIP
library and no device: the program supplies malloc-backed hipMalloc / hipFree / hipHostMalloc / hipHostFree /
hipHostGetDevicePointer that count live blocks and fail on request). The program checks growth, failure
and move semantics and exits non-zero on a mismatch or a leaked block; a sanitizer report aborts it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_devbuf_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    if not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime_api.h")):
        pytest.skip("no hip/hip_runtime_api.h")
    exe = str(tmp_path / "devbuf_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE,
                           "-o", exe, os.path.join(ROOT, "tests", "host", "devbuf_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "devbuf sanitizer run ok" in r.stdout
