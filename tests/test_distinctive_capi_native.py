"""A C++11 caller of plvi_distinctive_descriptors[_batch] (tests/native/distinctive_capi_check.cpp) that includes
only include/plvi_frontend.h, the way the INTEGRATION.md shims of MapPoint / MapLine::ComputeDistinctiveDescriptors
do: it compiles and links on the CPU host, and on the GPU its results equal the host restatement's
(tests/test_distinctive.py)."""
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_distinctive as td

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "distinctive_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "distinctive_capi_check"


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_distinctive_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout
    for name in ("plvi_distinctive_descriptors", "plvi_distinctive_descriptors_batch"):
        assert name in out.split()


def test_header_limit_matches_the_python_mirror():
    txt = plvi.HEADER_PATH.read_text()
    assert f"#define PLVI_DISTINCTIVE_MAX_OBS {plvi.DISTINCTIVE_MAX_OBS} " in txt
    assert plvi.DISTINCTIVE_MAX_OBS >= 1448  # no reference run can have produced a longer list


@pytest.mark.gpu
def test_distinctive_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    counts = np.random.default_rng(21).integers(0, 31, 200)
    counts[[3, 50]] = [70, 130]
    pool, off, rows = td.seeded(21, counts)
    rows = rows.copy()
    rows[::17] = -1  # absent leftIndex / rightIndex entries
    n, bp, bm, out = td.ref(pool, off, rows)
    assert n >= 190 and (bp > 0).sum() >= 50
    src = tmp_path / "in.bin"
    src.write_bytes(np.array([len(counts), len(pool), len(rows)], np.int32).tobytes() + pool.tobytes() +
                    off.tobytes() + rows.tobytes())
    dst = tmp_path / "out.bin"
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=120)
    raw = dst.read_bytes()
    nf = len(counts)
    words = np.frombuffer(raw[:4 + 8 * nf], np.int32)
    assert words[0] == n
    assert np.array_equal(words[1:1 + nf], bp) and np.array_equal(words[1 + nf:], bm)
    assert np.array_equal(np.frombuffer(raw[4 + 8 * nf:4 + 40 * nf], np.uint8).reshape(nf, 32), out)
    assert np.frombuffer(raw[4 + 40 * nf:], np.int32).tolist() == [0, td.E_CAPACITY, td.E_BADARG]
