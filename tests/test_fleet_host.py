"""CPU: the fleet-wide decentralized tick (tsw_nearby / tsw_decide_fleet, ABI 8) is declared in every
mirror of the C ABI, and the binned list construction of tsw_nearby.hip — restated in numpy — equals the
brute-force definition on every shape the GPU test runs (clipping and index mistakes show here first)."""
import ctypes
import os
import re

import numpy as np
import pytest

import p2p_distributed_tswap_amd as pkg

import fleet_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsw_nearby", "tsw_decide_fleet")


def test_fleet_entry_points_declared_everywhere():
    hdr = open(os.path.join(ROOT, "include", "tswap.h")).read()
    rs = open(os.path.join(ROOT, "rust", "tswap-amd-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in pkg.EXPORTED_SYMBOLS
        assert re.search(rf"\bint {name}\(tsw_ctx \*ctx", hdr), name
        assert re.search(rf"pub fn {name}\(ctx: \*mut TswCtx", rs), name
    assert re.search(r"pub fn nearby\(&mut self", rs) and re.search(r"pub fn decide_fleet\(&mut self", rs)
    assert hasattr(pkg.Planner, "nearby") and hasattr(pkg.Planner, "decide_fleet")
    # the header says which list order the library chose
    assert "ASCENDING AGENT INDEX" in hdr and "HashMap" in hdr


def test_abi_is_8_everywhere():
    hdr = open(os.path.join(ROOT, "include", "tswap.h")).read()
    rs = open(os.path.join(ROOT, "rust", "tswap-amd-sys", "src", "lib.rs")).read()
    assert re.search(r"#define TSW_ABI_VERSION 8\b", hdr)
    assert re.search(r"pub const TSW_ABI_VERSION: c_int = 8;", rs)
    assert pkg.TSW_ABI_VERSION == 8


def test_library_exports_fleet_entry_points():
    if not os.path.exists(pkg.LIB_PATH):
        pytest.skip("libtswap_hip.so not built (run __graft_entry__.build())")
    for path in (pkg.LIB_PATH, pkg.DIAG_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(lib, name), (path, name)
        lib.tsw_abi_version.restype = ctypes.c_int
        assert lib.tsw_abi_version() == 8


@pytest.mark.parametrize("name,r", fc.NEARBY_CASES)
def test_binned_construction_equals_brute_force(name, r):
    W, H, _, v = fc.nearby_shape(name)
    off, idx = fc.binned_nearby(v, W, H, r)
    boff, bidx = fc.brute_case(name, r)
    assert np.array_equal(off, boff)
    assert np.array_equal(idx, bidx)


def test_brute_force_shapes_cover_the_paths():
    """The shapes reach what they are there for: lists past the 1,024-entry LDS sort, co-located agents,
    empty lists, clipping on every side."""
    off, _ = fc.brute_case("open40", 80)
    assert np.all(np.diff(off.astype(np.int64)) == 1099)
    off, _ = fc.brute_case("open6", 0)
    assert 0 < off[-1] < 18 * 17  # r = 0: only the duplicates see anyone
    off, _ = fc.brute_case("edges13x7", 40)
    n = fc.nearby_shape("edges13x7")[3].size
    assert off[-1] == n * (n - 1)  # r > W + H: everyone
    assert fc.brute_case("one", 15)[0].tolist() == [0, 0] and fc.brute_case("none", 15)[0].tolist() == [0]
