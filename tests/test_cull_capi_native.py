"""A C++11 caller of plvi_keyframe_culling[_batch] (tests/native/cull_capi_check.cpp) that includes only
include/plvi_frontend.h, the way the INTEGRATION.md shim of LocalMapping::KeyFrameCullingWithLines does: it compiles
and links on the CPU host, the header's constants and struct sizes are the Python mirror's, and on the GPU the host
form and the batch form both equal the host restatement (tests/test_cull.py) on a random map with lines."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_cull as tc

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "cull_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "cull_capi_check"
NAMES = ("plvi_keyframe_culling", "plvi_keyframe_culling_batch", "plvi_keyframe_culling_scratch_bytes")


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_cull_capi_check_compiles_and_links():
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
    assert [int(x) for x in got] == [plvi.CULL_MAX_CHANGED, plvi.CULL_SPEC, plvi.CULL_NEEDS_NORM, plvi.CULL_DEFERRED,
                                     plvi.CULL_ERR_QUERY, ctypes.sizeof(plvi.CullKeyframes),
                                     ctypes.sizeof(plvi.CullFeatures), ctypes.sizeof(plvi.CullParams),
                                     ctypes.sizeof(plvi.CullQueries), ctypes.sizeof(plvi.CullOutputs)]
    # the overlay in LDS: the changed list, three link entries a relink, the filter -- a few KB
    assert plvi.CULL_MAX_CHANGED * 8 + 3 * plvi.CULL_MAX_CHANGED * 12 + 256 <= 8 * 1024
    assert plvi.CULL_SPEC == 101 and plvi.CULL_MAX_CHANGED >= 101   # count > 100 breaks; a cull does not `continue`


def lines_case():
    """A random non-inertial map with lines on which the walk culls."""
    for seed in range(1, tc.N_RANDOM, 4):
        m, P, Q, ref, _ = tc.random_ref(seed)
        if m.cap[1] and not P["inertial"] and not any(m.null_nobs) and ref["n_changed"] >= 2 and \
                float(P["redundant_th"]) == np.float32(0.9):
            return m, P, Q
    raise AssertionError("no such map")


def test_the_map_of_the_gpu_part_has_lines_and_culls():
    m, P, Q = lines_case()
    oc, cc = tc.caps_of(m)
    ref = tc.ref_walk(m.tables(), P, Q, oc, cc)
    assert tc.K_POINTS | tc.K_LINES in ref["changed_kind"] and ref["err"] == 0


@pytest.mark.gpu
def test_cull_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    m, P, Q = lines_case()
    kf, mp, ml = m.tables()
    oc, cc = tc.caps_of(m)
    want = tc.ref_walk((kf, mp, ml), P, Q, oc, cc)
    assert want["n_changed"] >= 2

    def blk(a, dt):
        b = np.ascontiguousarray(a, dt).tobytes()
        return np.array([len(b)], np.int32).tobytes() + b
    i32, u8 = np.int32, np.uint8
    blob = blk([m.K, m.cap[0], m.cap[1], kf["cand"].shape[1], len(mp["bad"]), len(ml["bad"]), Q["q_slot"],
                Q["n_kf_in_map"], oc, cc, P["monocular"], P["slam_mode"]], i32)
    for a, dt in ((kf["bad"], u8), (kf["init_kf"], u8), (kf["not_erase"], u8), (kf["mp"], i32), (kf["nmp"], i32),
                  (kf["kp_info"], u8), (kf["ml"], i32), (kf["nml"], i32), (kf["kl_info"], u8), (kf["cand"], i32),
                  (kf["n_cand"], i32)):
        blob += blk(a, dt)
    for p in (mp, ml):
        for k, dt in (("bad", u8), ("obs_off", i32), ("obs_kf", i32), ("obs_idx", i32), ("nobs", i32)):
            blob += blk(p[k], dt)
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
        assert take(i32) == [want[k] for k in tc.PER_Q], form
        for k in tc.PER_C + tc.PER_CH:
            assert take(u8 if k == "outcome" else i32) == want[k], (form, k)
    assert take(i32) == [tc.E_BADARG, tc.E_BADARG, tc.E_CAPACITY, 256 + 2 * 16 * plvi.CULL_SPEC]
    assert pos == len(raw)
