#!/usr/bin/env python3
"""Round trip between a running kernel and a host thread through mapped coherent host memory
(scripts/host_pingpong.hip): the transport of the host A* service. Builds scripts/bin/host_pingpong
if it is missing, runs it and writes its report.

    python scripts/host_pingpong.py [--trips 1000] [--out profiles/r7/host_pingpong.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "scripts", "host_pingpong.hip")
EXE = os.path.join(ROOT, "scripts", "bin", "host_pingpong")


def build() -> None:
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= os.path.getmtime(SRC):
        return
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-o", EXE, SRC])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--trips", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    build()
    if a.build_only:
        return 0
    r = subprocess.run([EXE, str(a.trips)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
