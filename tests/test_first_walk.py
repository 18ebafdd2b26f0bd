"""The first-occurrence walk of csrc/first_walk.h (KfTable, first_mark, row_walk, first_compact) and the attribute
gather of csrc/map_pool.h against the host, each in a small kernel of its own: tests/native/first_walk_check.hip."""
import pathlib
import subprocess

import pytest

from test_block_prims import CSRC, FLAGS, ROOT

SRC = ROOT / "tests" / "native" / "first_walk_check.hip"
BIN = ROOT / "tests" / "native" / "_build" / "first_walk_check"


def build_first_walk_check():
    deps = [SRC] + [CSRC / h for h in ("first_walk.h", "block_prims.h", "map_pool.h", "host_stage.h", "plvi_common.h")]
    if not BIN.exists() or BIN.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        BIN.parent.mkdir(exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", str(BIN), str(SRC)], check=True)
    return str(BIN)


def test_first_walk_check_builds():
    """The header compiles for gfx950 on its own, with the library's flags (no device needed)."""
    assert pathlib.Path(build_first_walk_check()).exists()


@pytest.mark.gpu
def test_first_walk_matches_host():
    """first_mark + first_compact<1024, 8> in one workgroup against a std::set first-come loop: the list, its order,
    the position reported per kept entry and the full count, with every output cell available and with half the count
    (cells past the capacity keep the fill).  cap 1, 3, 8, 13, 64 by 0, 1, 2, 6, 31 rows, and totals of 8191, 8192,
    8193 (cap 1 and cap 3 x 2731) and 16389 positions around the 8192-position scan block; per-row lengths 0, cap, in
    between, negative and above cap; ids -1, >= n, bad, repeated within and across rows; a pool of 50 ids and one
    larger than the walk; with and without an extra predicate; the table starting as 0xA5 garbage with reset and as
    "none" without.  first_mark alone over a 6 x 5 functor with repeats, and PoolGather on 0, 1, 255, 256, 257 rows
    with all and some destinations set, against host copies."""
    r = subprocess.run([build_first_walk_check()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
