"""A C++11 caller of the Fuse searches of the C-ABI (tests/native/fuse_capi_check.cpp) that includes only
include/plvi_frontend.h, the way the INTEGRATION.md shims of LocalMapping::SearchInNeighbors /
LoopClosing::SearchAndFuse do: it compiles and links on the CPU host, and on the GPU its ORBmatcher::Fuse (both
overloads) and LineMatcher::Fuse results equal the host restatement's (tests/test_fuse.py)."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_fuse as tf

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "fuse_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "fuse_capi_check"


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_fuse_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout
    for name in ("plvi_fuse_points", "plvi_fuse_points_batch", "plvi_fuse_lines", "plvi_fuse_lines_batch"):
        assert name in out.split()


@pytest.mark.gpu
def test_fuse_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    th = 3.0
    c, _ = tf.points_general_cached(tf.POINTS_GENERAL[0])
    l, _ = tf.lines_general_cached(tf.LINES_GENERAL[0])
    refs = [tf.ref_points(c, mode, th) for mode in (0, 1)] + [tf.ref_lines(l, th)]
    assert all(r[0] >= 20 for r in refs)
    n_kp, n_pt, n_kl, n_ml = len(c["kps"]), len(c["flags"]), len(l["kl"]), len(l["flags"])
    assert ctypes.sizeof(plvi.FuseParams) == 184 and ctypes.sizeof(plvi.FuseLineParams) == 104
    parts = [np.array([n_kp, n_pt, 1, n_kl, n_ml], np.int32), bytes(tf.fuse_params(c, 0, th)), c["kps"], c["desc"],
             c["uright"]] + [c[k] for k in tf.PT_KEYS] + [bytes(tf.line_params(l, th)), l["kl"], l["kl_desc"]] + \
        [l[k] for k in tf.ML_KEYS]
    src = tmp_path / "in.bin"
    src.write_bytes(b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts))
    out = tmp_path / "out.bin"
    subprocess.run([str(exe), str(src), str(out)], check=True, timeout=120)
    words = np.frombuffer(out.read_bytes(), np.int32)
    pos = 0
    for (ne, ie, de, _), rows in zip(refs, (n_pt, n_pt, n_ml)):
        assert words[pos] == ne
        assert np.array_equal(words[pos + 1:pos + 1 + rows], ie)
        assert np.array_equal(words[pos + 1 + rows:pos + 1 + 2 * rows], de)
        pos += 1 + 2 * rows
    assert words[pos:].tolist() == [0, 0]
