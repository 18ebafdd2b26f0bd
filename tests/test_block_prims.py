"""The wave / workgroup primitives of csrc/block_prims.h (hamming256, wave_sum, wave_incl_scan,
block_scan, block_add, block_scan_array, bitonic_sort, pow2_at_least) against the host, each in a one-workgroup
kernel: tests/native/block_prims_check.hip."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "pl-vi-orbslam3_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "block_prims_check.hip"
BIN = ROOT / "tests" / "native" / "_build" / "block_prims_check"
# the library's flags (pl-vi-orbslam3_amd/Makefile)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
         "-Wno-unused-function", "-Wno-unused-variable", "-I" + str(ROOT / "include")]


def build_block_prims_check():
    deps = [SRC, CSRC / "block_prims.h", CSRC / "plvi_common.h"]
    if not BIN.exists() or BIN.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        BIN.parent.mkdir(exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", str(BIN), str(SRC)], check=True)
    return str(BIN)


def test_block_prims_check_builds():
    """The header compiles for gfx950 on its own, with the library's flags (no device needed)."""
    assert pathlib.Path(build_block_prims_check()).exists()


@pytest.mark.gpu
def test_block_prims_match_host():
    """block_scan<1, 4, 8, 16> twice back to back through one s_wave (all zero / all one / a 0, 1, large mix),
    block_add into two counters by 1, 4 and 16 waves (all zero / all one / a mix with a wave of zeros),
    block_scan_array at n = 0, 1, 255, 256, 257, 481, 3073, bitonic_sort of unsigned and 64-bit keys with and
    without a carried val at n = 2, 256, 512, 8192 by 64, 256 and 1024 threads (duplicates, a ~0 padding tail;
    with val every (key, val) pair survives), both hamming256 overloads at distances 0, 1, 255, 256 and others,
    wave_sum and wave_incl_scan: all equal to std::partial_sum / std::sort / a bit loop."""
    r = subprocess.run([build_block_prims_check()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
