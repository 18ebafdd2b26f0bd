"""A C++11 caller of plvi_gba_walk[_device] and plvi_gba_correct[_device]
(tests/native/gba_propagate_capi_check.cpp) that includes only include/plvi_frontend.h, the way the INTEGRATION.md
shim of RunGlobalBundleAdjustment's second half does: it compiles and links on the CPU host, the header's constants
and struct sizes are the Python mirror's, and on the GPU the host forms and the device forms (the correction writing
the pool's own column) both equal the host restatement (tests/test_gba_propagate.py)."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_gba_propagate as tg

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "gba_propagate_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "gba_propagate_capi_check"
NAMES = ("plvi_gba_walk", "plvi_gba_walk_device", "plvi_gba_walk_scratch_bytes", "plvi_gba_correct",
         "plvi_gba_correct_device")
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


def test_gba_propagate_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout.split()
    for name in NAMES:
        assert name in out


def test_header_constants_and_struct_sizes_match_the_python_mirror():
    declared = set(plvi.exported_symbols())
    lib = plvi.load()
    for name in NAMES:
        assert name in declared and getattr(lib, name).argtypes is not None
    U, V, I, S = ctypes.c_uint, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    sig = plvi.signatures()
    assert sig["plvi_gba_walk_device"] == ([V, V, V, I, U, V, V, V, S, V], I)      # loop_kf is an unsigned
    assert sig["plvi_gba_walk_scratch_bytes"] == ([I], S)
    got = subprocess.run([str(build()), "--sizes"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [plvi.GBA_POINTS, plvi.GBA_LINES, plvi.GBA_ERR_ORIGIN, plvi.GBA_ERR_CYCLE,
                                     plvi.GBA_ERR_WALK, plvi.GBA_ERR_REF, plvi.COMPAT_GEMM_FMA,
                                     ctypes.sizeof(plvi.GbaWalkOutputs), ctypes.sizeof(plvi.GbaPoses),
                                     ctypes.sizeof(plvi.GbaParams), ctypes.sizeof(plvi.GbaCorrectOutputs)]


def test_scratch_bytes_contract():
    f = plvi.load().plvi_gba_walk_scratch_bytes
    assert f(-1) == 0
    # the rank, the first position, the usable count, the sorted rows and the queue, each rounded up to 256 bytes
    assert f(100) == 5 * 512 and f(0) == 0 and f(64) == 5 * 256 and f(65) == 5 * 512


@pytest.mark.gpu
def test_gba_propagate_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    i32, u32, u8, f32 = np.int32, np.uint32, np.uint8, np.float32
    kf, origins, _ = tg.walk_cases()["descending_rows_permuted_order_300"]
    origins = np.array(origins + [300], i32)        # the host form reports the raised bit
    K = len(kf["bad"])
    exp_w = tg.ref_walk(kf, origins)
    assert exp_w["err"] == tg.E_ORIGIN and exp_w["n_walk"] == 300
    m = tg.feature_map(tg.POINTS, 500, K=K, seed=4)
    f, p = m["feat"], m["poses"]
    exp_c = tg.ref_correct(m, tg.FMA)
    assert exp_c["err"] == 0 and (exp_c["counts"] > 20).all()

    def blk(a, dt):
        b = np.ascontiguousarray(a, dt).tobytes()
        return np.array([len(b)], i32).tobytes() + b
    blob = blk([K, len(kf["order"]), len(origins), tg.LOOP, 500, m["map"], tg.FMA, K], i32)
    for a, dt in ((kf["bad"], u8), (kf["order"], i32), (kf["child_off"], i32), (kf["child"], i32), (origins, i32),
                  (kf["kf_ba_for"], u32), (f["bad"], u8), (f["ref_kf"], i32), (f["map_id"], i32), (f["ba_for"], u32),
                  (f["pos_gba"], f32), (f["pos"], f32), (p["kf_ba_for"], u32), (p["has_bef"], u8), (p["tcw_bef"], f32),
                  (p["twc"], f32)):
        blob += blk(a, dt)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=120)
    raw, pos = dst.read_bytes(), 0

    def take(dt=i32):
        nonlocal pos
        n = int(np.frombuffer(raw, i32, 1, pos)[0])
        pos += 4 + n
        return np.frombuffer(raw[pos - n:pos], dt)
    sb = plvi_lib.plvi_gba_walk_scratch_bytes(K)
    for form in ("host", "device"):
        if form == "device":
            assert take().tolist() == [E_BADARG, E_BADARG, E_BADARG, E_BADARG, E_BADARG, 0, sb]
        assert take()[0] == (E_CAPACITY if form == "host" else 0), form
        n_walk, n_new, err = take().tolist()
        got = dict(n_walk=n_walk, n_new=n_new, err=err, walk=take(), walk_parent=take(), walk_new=take(u8),
                   visited=take(u8), kf_ba_for=take(u32))
        want = {k: (v[:K] if k in ("walk", "walk_parent", "walk_new") else v) for k, v in exp_w.items()}
        tg.same_walk(got, want)
        assert take()[0] == (int(exp_c["counts"][1] + exp_c["counts"][2]) if form == "host" else 0), form
        cs = take()
        got = dict(counts=cs[:3], err=cs[3], pos=take(f32).reshape(-1, 3), state=take(u8))
        tg.same_correct(got, dict(exp_c, state=exp_c["state"][:500]), "pos")
    assert pos == len(raw)
