"""A C++11 caller of plvi_feature_refresh[_batch] (tests/native/feature_refresh_capi_check.cpp) that includes only
include/plvi_frontend.h, the way the INTEGRATION.md shim of UpdateNormalAndDepth + ComputeDistinctiveDescriptors does:
it compiles and links on the CPU host, the header's constants and struct sizes are the Python mirror's, and on the GPU
the host form and the device form (writing the pool's own columns) both equal the host restatement
(tests/test_feature_refresh.py) on a random map."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_feature_refresh as tf

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "feature_refresh_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "feature_refresh_capi_check"
NAMES = ("plvi_feature_refresh", "plvi_feature_refresh_batch", "plvi_feature_refresh_scratch_bytes")
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


def test_feature_refresh_capi_check_compiles_and_links():
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
    assert [int(x) for x in got] == [plvi.REFRESH_POINTS, plvi.REFRESH_LINES, plvi.REFRESH_NORMAL, plvi.REFRESH_DESC,
                                     plvi.REFRESH_ERR_ROWS, plvi.REFRESH_ERR_REF, plvi.REFRESH_ERR_LEVEL,
                                     plvi.REFRESH_ERR_KEYPOINT, plvi.REFRESH_MAX_LEVELS, plvi.COMPAT_SCALEADD_FMA,
                                     ctypes.sizeof(plvi.RefreshKeyframes), ctypes.sizeof(plvi.RefreshParams),
                                     ctypes.sizeof(plvi.RefreshOutputs)]


def test_scratch_bytes_contract():
    f = plvi.load().plvi_feature_refresh_scratch_bytes
    assert f(-1, 1) == 0 and f(1, -1) == 0
    # the offsets, the rows, best_pos, best_median and a 32-byte row per id, each rounded up to 256 bytes
    assert f(100, 1000) == 512 + 4096 + 512 + 512 + 3328
    assert f(0, 0) == 256 + 0 + 0 + 0 + 0


@pytest.mark.gpu
def test_feature_refresh_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    tabs, ids = tf.random_case(tf.POINTS)
    kf, feat, scale = tabs
    ids = np.array(ids, np.int32)
    max_obs = tf.max_obs_of(tabs)
    exp = tf.ref_refresh(tabs, tf.POINTS, ids, compat=tf.FMA)
    assert exp["err"] == tf.E_REF and (exp["state"] == 3).sum() > 100   # the host form reports the raised bit

    def blk(a, dt):
        b = np.ascontiguousarray(a, dt).tobytes()
        return np.array([len(b)], np.int32).tobytes() + b
    i32, u8, f32 = np.int32, np.uint8, np.float32
    blob = blk([len(kf["bad"]), kf["info"].shape[1], len(feat["bad"]), len(ids), max_obs, exp["n_rows"], tf.FMA,
                len(scale)], i32) + blk(scale, f32)
    for k, dt in (("bad", u8), ("ow", f32), ("cnt", i32), ("info", u8), ("desc", u8)):
        blob += blk(kf[k], dt)
    for k, dt in (("bad", u8), ("obs_off", i32), ("obs_kf", i32), ("obs_idx", i32), ("ref_kf", i32), ("pos", f32),
                  ("normal", f32), ("dist", f32), ("desc", u8)):
        blob += blk(feat[k], dt)
    blob += blk(ids, i32)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=120)
    raw, pos = dst.read_bytes(), 0

    def take(dt=i32):
        nonlocal pos
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0])
        pos += 4 + n
        return np.frombuffer(raw[pos - n:pos], dt)
    for form in ("host", "device"):
        assert take()[0] == (E_CAPACITY if form == "host" else 0), form
        n_rows, err = take().tolist()
        got = dict(n_rows=n_rows, err=err, normal=take(f32).reshape(-1, 3), dist=take(f32).reshape(-1, 2),
                   desc=take(u8).reshape(-1, 32), state=take(u8), best_pos=take(), best_median=take())
        tf.same(got, exp)
    sb = plvi_lib.plvi_feature_refresh_scratch_bytes(len(ids), exp["n_rows"])
    assert take().tolist() == [E_BADARG, E_BADARG, E_CAPACITY, E_BADARG, E_BADARG, E_BADARG, 0, sb]
    assert pos == len(raw)
