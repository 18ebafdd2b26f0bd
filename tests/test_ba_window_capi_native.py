"""A C++11 caller of plvi_ba_window[_batch] (tests/native/ba_window_capi_check.cpp) that includes only
include/plvi_frontend.h, the way the INTEGRATION.md shim of Optimizer::LocalBundleAdjustment does: it compiles and
links on the CPU host, the header's constants and struct sizes are the Python mirror's, and on the GPU the host form
and the batch form both equal the host restatement (tests/test_ba_window.py) on a crafted query with two moves."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_ba_window as tb

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "ba_window_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "ba_window_capi_check"
NAMES = ("plvi_ba_window", "plvi_ba_window_batch", "plvi_ba_window_scratch_bytes")
E_BADARG, E_CAPACITY = -2, -3


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_ba_window_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout.split()
    for name in NAMES:
        assert name in out


def test_header_constants_and_struct_sizes_match_the_python_mirror():
    declared = set(plvi.exported_symbols())
    lib = plvi.load()
    for name in NAMES:
        assert name in declared and getattr(lib, name).argtypes is not None
    got = subprocess.run([str(build()), "--sizes"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [plvi.BA_LDS_KF, plvi.BA_MAX_OPT, plvi.BA_MAX_FIXED_INERTIAL, plvi.BA_INERTIAL,
                                     plvi.BA_EDGE_LINE, plvi.BA_ERR_QUERY, ctypes.sizeof(plvi.BAFeatures),
                                     ctypes.sizeof(plvi.BAParams), ctypes.sizeof(plvi.BAQueries),
                                     ctypes.sizeof(plvi.BAOutputs)]
    # keys[] and cam[] at the LDS bound: 8 + 4 bytes a slot, keys padded to a power of two
    assert plvi.BA_LDS_KF & (plvi.BA_LDS_KF - 1) == 0 and 12 * plvi.BA_LDS_KF <= 32 * 1024
    assert plvi.BA_MAX_OPT >= 25 and plvi.BA_MAX_FIXED_INERTIAL == 200


def test_scratch_bytes_contract():
    f = plvi.load().plvi_ba_window_scratch_bytes
    assert f(-1, 10, 5, 5) == 0 and f(1, 0, 5, 5) == 0 and f(1, 10, -1, 0) == 0
    one, two = f(1, 100, 1000, 300), f(2, 100, 1000, 300)
    assert two - one == one - f(0, 100, 1000, 300) >= 8 * 128 + 4 * 100 * 2 + 2 * 4 * 1000
    assert f(1, 100, 300, 1000) == one, "the larger pool decides"


@pytest.mark.gpu
def test_ba_window_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    tabs, cases = tb.crafted(tb.POINTS)
    kf, mp, kf_map = tabs
    q = cases["two_moves"][0]
    caps = tb.big_caps(tabs)
    want = tb.ref_window(tabs, tb.POINTS, q, 0, caps=caps)
    assert want["num_fixed"] == 2 and want["n_fixed_kf"] == 2

    def blk(a, dt):
        b = np.ascontiguousarray(a, dt).tobytes()
        return np.array([len(b)], np.int32).tobytes() + b
    i32, u8 = np.int32, np.uint8
    blob = blk([len(kf["bad"]), kf["mp"].shape[1], kf["cand"].shape[1], len(mp["bad"]), q] +
               [caps[c] for c in tb.CAPS], i32)
    for a, dt in ((kf["bad"], u8), (kf["init_kf"], u8), (kf["mp"], i32), (kf["nmp"], i32), (kf["kp_info"], u8),
                  (kf["cand"], i32), (kf["n_cand"], i32), (kf["kf_id"], np.uint32), (kf_map, i32), (mp["bad"], u8),
                  (mp["obs_off"], i32), (mp["obs_kf"], i32), (mp["obs_idx"], i32), (mp["map_id"], i32)):
        blob += blk(a, dt)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=120)
    raw, pos = dst.read_bytes(), 0

    def take(dt):
        nonlocal pos
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0])
        pos += 4 + n
        return np.frombuffer(raw[pos - n:pos], dt).tolist()
    for form in ("host", "batch"):
        assert take(i32) == [want[k] for k in tb.SCALARS], form
        for k in tb.LISTS:
            assert take(u8 if k == "edge_kind" else i32) == want[k], (form, k)
    sb2 = plvi_lib.plvi_ba_window_scratch_bytes(2, len(kf["bad"]), len(mp["bad"]), 0)
    assert take(i32) == [E_BADARG, E_BADARG, E_CAPACITY, E_BADARG, sb2]
    assert pos == len(raw)
