"""A C++11 caller of the triangulation section of the C-ABI
(tests/native/triangulation_capi_check.cpp) that includes only
include/plvi_frontend.h, the way the INTEGRATION.md shims of
LocalMapping::CreateNewMapPoints / CreateNewMapLines do: it compiles and
links on the CPU host, and on the GPU its SearchForTriangulation results for
points and lines equal the host restatement's (tests/test_triangulation.py)."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_triangulation as tt

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "triangulation_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "triangulation_capi_check"


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_triangulation_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout
    for name in ("plvi_search_for_triangulation", "plvi_line_search_triangulation_batch"):
        assert name in out


@pytest.mark.gpu
def test_triangulation_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    c, (ne, me, _) = tt.general(0)
    d1, d2 = tt.line_case(21)
    h1, h2 = tt.line_masks(d1, d2)
    pe, made = tt.ref_lines(d1, d2, h1, h2)
    a, ao, ai = plvi.feature_vector_csr(c["fv1"])
    b, bo, bi = plvi.feature_vector_csr(c["fv2"])
    n1, n2 = len(c["kps1"]), len(c["kps2"])
    parts = [np.array([n1, n2, len(a), len(b), len(d1), len(d2)], np.int32), bytes(tt.pair_of(c)),
             c["kps1"], c["desc1"], a, ao, ai, c["has1"], c["ur1"], c["kps2"], c["desc2"], b, bo, bi, c["has2"],
             c["ur2"], d1, d2, h1, h2]
    assert ctypes.sizeof(plvi.TriangulationPair) == 192
    src = tmp_path / "in.bin"
    src.write_bytes(b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts))
    out = tmp_path / "out.bin"
    subprocess.run([str(exe), str(src), str(out)], check=True, timeout=120)
    buf = out.read_bytes()
    nm = int(np.frombuffer(buf, np.int32, 1)[0])
    m12 = np.frombuffer(buf, np.int32, n1, 4)
    off = 4 + 4 * n1
    lrc, npairs = np.frombuffer(buf, np.int32, 2, off).tolist()
    pairs = np.frombuffer(buf, np.int32, 2 * len(d1), off + 8).reshape(-1, 2)
    mad = np.frombuffer(buf, np.float64, 2, off + 8 + 8 * len(d1))
    assert nm == ne and np.array_equal(m12, me)
    assert lrc == 0 and npairs == len(pe) and np.array_equal(pairs[:npairs], pe) and tuple(mad) == made
