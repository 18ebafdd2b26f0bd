"""A C++11 caller of the loop-closing matchers of the C-ABI (tests/native/loop_match_capi_check.cpp) that
includes only include/plvi_frontend.h, the way the INTEGRATION.md shims of
LoopClosing::DetectCommonRegionsFromBoW / FindMatchesByProjection do: it compiles and links on the CPU host,
and on the GPU its SearchByBoW(KF, KF) and SearchByProjection(pKF, Scw, ...) results equal the host
restatement's (tests/test_loop_match.py)."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_loop_match as lm

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "loop_match_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "loop_match_capi_check"


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_loop_match_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout
    for name in ("plvi_search_by_bow_kf", "plvi_search_by_bow_kf_batch", "plvi_search_sim3_projection",
                 "plvi_search_sim3_projection_batch"):
        assert name in out.split()


@pytest.mark.gpu
def test_loop_match_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    c, (ne, me, _) = lm.bow_general_cached(0)
    s, refs = lm.sim3_general_cached(lm.SIM3_GENERAL[0])
    call = lm.LOOP_CALLS[0]
    npe, mpe = refs[call][:2]
    a, ao, ai = plvi.feature_vector_csr(c["fv1"])
    b, bo, bi = plvi.feature_vector_csr(c["fv2"])
    n1, n2, n_kp, n_pt = len(c["desc1"]), len(c["desc2"]), len(s["cur_kps"]), len(s["kf_flags"])
    assert ctypes.sizeof(plvi.Sim3ProjParams) == 120
    parts = [np.array([n1, n2, len(a), len(b), int(c["ori"]), n_kp, n_pt, 1], np.int32),
             np.array([c["nnratio"]], np.float32), c["desc1"], c["angle1"], c["live1"], a, ao, ai, c["desc2"],
             c["angle2"], c["live2"], b, bo, bi, bytes(lm.sim3_params(s, *call)), s["cur_kps"], s["cur_desc"],
             s["cur_blocked"], s["kf_flags"], s["x3dc"], s["dist"], s["dot"], s["level"], s["mp_desc"]]
    src = tmp_path / "in.bin"
    src.write_bytes(b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts))
    out = tmp_path / "out.bin"
    subprocess.run([str(exe), str(src), str(out)], check=True, timeout=120)
    buf = out.read_bytes()
    nb = int(np.frombuffer(buf, np.int32, 1)[0])
    m12 = np.frombuffer(buf, np.int32, n1, 4)
    off = 4 + 4 * n1
    npj = int(np.frombuffer(buf, np.int32, 1, off)[0])
    match = np.frombuffer(buf, np.int32, n_kp, off + 4)
    rcs = np.frombuffer(buf, np.int32, 2, off + 4 + 4 * n_kp).tolist()
    assert nb == ne and np.array_equal(m12, me)
    assert npj == npe and np.array_equal(match, mpe)
    assert rcs == [0, 0]
