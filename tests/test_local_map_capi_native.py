"""A C++11 caller of the plvi_local_map_* entry points (tests/native/local_map_capi_check.cpp) that includes only
include/plvi_frontend.h, the way the INTEGRATION.md shim of Tracking::UpdateLocalMap does: it compiles and links on
the CPU host, and on the GPU the host form and the batch form both equal the host restatement
(tests/test_local_map.py)."""
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_local_map as tl

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "local_map_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "local_map_capi_check"
NAMES = ("plvi_local_map", "plvi_local_map_batch", "plvi_local_map_scratch_bytes")


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_local_map_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout.split()
    for name in NAMES:
        assert name in out


def test_header_limits_match_the_python_mirror():
    txt = plvi.HEADER_PATH.read_text()
    assert f"#define PLVI_LOCAL_MAP_LDS_KF {plvi.LOCAL_MAP_LDS_KF} " in txt
    assert f"#define PLVI_LOCAL_MAP_GROUP_ENTRIES {plvi.LOCAL_MAP_GROUP_ENTRIES} " in txt
    assert f"#define PLVI_LOCAL_MAP_MAX_GROUPS {plvi.LOCAL_MAP_MAX_GROUPS}\n" in txt
    assert f"#define PLVI_LOCAL_MAP_MAX_ENTRIES {plvi.LOCAL_MAP_MAX_ENTRIES:#x} " in txt
    # the histogram (4 B a slot) and the listed-set (1 bit a slot) share a workgroup's 64 KB of LDS
    assert plvi.LOCAL_MAP_LDS_KF * 4 + plvi.LOCAL_MAP_LDS_KF // 8 <= 60 * 1024
    declared = set(plvi.exported_symbols())
    for name in NAMES:
        assert name in declared
    # the ctypes mirrors have the size the C structs have on this ABI: 4-byte ints, 8-byte pointers, padded to 8
    import ctypes
    assert ctypes.sizeof(plvi.LocalMapKeyframes) == 16 + 11 * 8
    assert ctypes.sizeof(plvi.LocalMapPool) == 8 + 8 * 8
    assert ctypes.sizeof(plvi.LocalMapFrames) == 4 * 24 + 8
    assert ctypes.sizeof(plvi.LocalMapOutputs) == 16 + 18 * 8


@pytest.mark.gpu
def test_local_map_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    m, frames, _, _ = tl.case_and_ref("random_lines")
    # a seen table of the frame's own (the IMU branch votes with the last frame's): half of the voting points,
    # a few ids that do not vote, a NULL
    frames = [dict(fr, seen_mp=fr["vote_mp"][::2] + [5 + f, 40 + f, -1]) for f, fr in enumerate(frames)]
    refs = [tl.ref_frame(m, fr) for fr in frames]
    assert all(0 < sum(1 for x in r["mp_flags"] if not x & 1) < len(r["mp_flags"]) for r in refs)
    kf, mp, ml = m.tables()
    args = tl.gpu_args(frames)
    B = len(frames)

    def blk(a, dt):
        b = np.ascontiguousarray(a, dt).tobytes()
        return np.array([len(b)], np.int32).tobytes() + b
    i32, u8 = np.int32, np.uint8
    blob = blk([m.K, len(kf["order"]), m.kp_cap, m.kl_cap, len(mp["bad"]), len(ml["bad"]), B,
                args["vote_mp"].shape[1], args["vote_ml"].shape[1], args["seen_mp"].shape[1]], i32)
    for a, dt in ((kf["bad"], u8), (kf["order"], i32), (kf["covis"], i32), (kf["child_off"], i32), (kf["child"], i32),
                  (kf["parent"], i32), (kf["prev_kf"], i32), (kf["mp"], i32), (kf["nmp"], i32), (kf["ml"], i32),
                  (kf["nml"], i32), (mp["bad"], u8), (mp["obs_off"], i32), (mp["obs_kf"], i32),
                  (mp["pos"], np.float32), (mp["desc"], u8), (ml["bad"], u8), (ml["obs_off"], i32),
                  (ml["obs_kf"], i32), (ml["sep"], np.float64), (args["vote_mp"], i32), (args["n_vote_mp"], i32),
                  (args["vote_ml"], i32), (args["n_vote_ml"], i32), (args["last_kf"], i32), (args["seen_mp"], i32),
                  (args["n_seen_mp"], i32)):
        blob += blk(a, dt)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=120)

    raw, pos = dst.read_bytes(), 0

    def take(dt):
        nonlocal pos
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0])
        pos += 4 + n
        return np.frombuffer(raw[pos - n:pos], dt)
    for form in ("host", "batch"):
        for f, r in enumerate(refs):
            ids, lids = np.array(r["local_mp"], np.int64), np.array(r["local_ml"], np.int64)
            assert take(i32).tolist() == [0, len(r["local_kf"]), r["ref_kf"], len(ids), len(lids), 0], (form, f)
            assert take(i32).tolist() == r["local_kf"]
            assert take(i32).tolist() == r["local_mp"]
            assert take(u8).tolist() == r["mp_flags"]
            assert np.array_equal(take(np.float32).reshape(-1, 3), mp["pos"][ids])
            assert np.array_equal(take(u8).reshape(-1, 32), mp["desc"][ids])
            assert take(i32).tolist() == r["local_ml"]
            assert np.array_equal(take(np.float64).reshape(-1, 6), ml["sep"][lids])
            for name in ("vote_mp", "vote_ml"):
                want = args[name][f].copy()
                want[:len(r[name])] = r[name]
                assert np.array_equal(take(i32), want), (form, f, name)
    assert take(i32).tolist() == [tl.E_BADARG, tl.E_BADARG, tl.E_BADARG, tl.E_CAPACITY, 0]
    assert pos == len(raw)
