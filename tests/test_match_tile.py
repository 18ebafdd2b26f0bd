"""The matrix-core kNN-2's key arithmetic (csrc/match_tile.h) on the host:
tests/native/match_tile_check.cpp replays the kernel's tile walk -- bit
expansion to int8 operands, int32 tile products, key packing, the masked tail
tile, the running top-2, the merge of the four lane groups and the sentinel
decode -- over random, near-duplicate, duplicate-heavy, all-equal and
all-zero / all-one tables and compares every query with a brute-force
BFMatcher scan.  No GPU."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "match_tile_check.cpp"
BIN = ROOT / "tests" / "native" / "_build" / "match_tile_check"
CSRC = ROOT / "pl-vi-orbslam3_amd" / "csrc"

# nq:nt -- tile edges on both sides, fewer than two trains, one tile exactly, several tiles with a tail
SIZES = ["1:1", "1:2", "2:1", "3:0", "15:17", "16:16", "17:15", "31:33", "64:64", "65:63", "20:300", "100:129"]
KINDS = 5


def test_tile_walk_matches_brute_force():
    BIN.parent.mkdir(exist_ok=True)
    hdr = CSRC / "match_tile.h"
    if not BIN.exists() or BIN.stat().st_mtime < max(SRC.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", f"-I{CSRC}", "-o", str(BIN), str(SRC)], check=True)
    r = subprocess.run([str(BIN), *SIZES], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches=0" in r.stdout
    n = 32 * 8 * 4 + KINDS * sum(int(s.split(":")[0]) for s in SIZES)
    assert f"checked={n} " in r.stdout
