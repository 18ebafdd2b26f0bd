"""A C++11 caller of plvi_loop_window[_batch] and plvi_loop_bow_merge[_batch]
(tests/native/loop_window_capi_check.cpp) that includes only include/plvi_frontend.h, the way the INTEGRATION.md shim
of LoopClosing::NewDetectCommonRegions does: it compiles and links on the CPU host, the header's constants and struct
sizes are the Python mirror's, and on the GPU the host forms and the batch forms both equal the host restatement
(tests/test_loop_window.py) on a crafted PROJ query with a gather and a crafted BOW query with its merge."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_loop_window as tl

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "loop_window_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "loop_window_capi_check"
NAMES = ("plvi_loop_window", "plvi_loop_window_batch", "plvi_loop_bow_merge", "plvi_loop_bow_merge_batch",
         "plvi_loop_window_scratch_bytes")
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


def test_loop_window_capi_check_compiles_and_links():
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
    assert [int(x) for x in got] == [plvi.LOOP_COVISIBLES, plvi.LOOP_BOW_WIN, plvi.LOOP_WIN_MAX, plvi.LOOP_WIN_LAST,
                                     plvi.LOOP_ERR_QUERY, ctypes.sizeof(plvi.LoopQueries),
                                     ctypes.sizeof(plvi.LoopOutputs)]
    # nNumCovisibles = 5: the BoW window is the candidate and five, the last window five, one and five times five
    assert plvi.LOOP_BOW_WIN == plvi.LOOP_COVISIBLES + 1
    assert plvi.LOOP_WIN_MAX == plvi.LOOP_COVISIBLES + 1 + plvi.LOOP_COVISIBLES ** 2


def test_scratch_bytes_contract():
    f = plvi.load().plvi_loop_window_scratch_bytes
    assert f(-1, 10) == 0 and f(1, -1) == 0
    assert f(0, 1000) == 256 and f(3, 1000) == 256 + 3 * 4000


@pytest.mark.gpu
def test_loop_window_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    tabs, cases = tl.crafted()
    kf, pool = tabs
    qa, qb = cases["proj-owner-and-bad-kf"][0], cases["merge-overwrite-and-first-cell"][0]
    qb = dict(qb, conn=[qb["cur_slot"], tl.OUT])      # a connected set that aborts nothing
    pt_cap = 6
    wa, wb = tl.ref_run(tabs, [qa, qb], pt_cap)
    assert wa["n_pts"] == 3 and wb["num"] == 3
    cap1 = qb["m12"].shape[1]

    def blk(a, dt):
        b = np.ascontiguousarray(a, dt).tobytes()
        return np.array([len(b)], np.int32).tobytes() + b
    i32, u8, f32 = np.int32, np.uint8, np.float32
    blob = blk([len(kf["bad"]), kf["mp"].shape[1], kf["cand"].shape[1], len(pool["bad"]), qa["kind"], qa["kf_slot"],
                pt_cap, qb["kf_slot"], qb["cur_slot"], qb["n1"], cap1], i32)
    for a, dt in ((kf["bad"], u8), (kf["mp"], i32), (kf["nmp"], i32), (kf["cand"], i32), (kf["n_cand"], i32),
                  (pool["bad"], u8), (pool["pos"], f32), (qb["conn"], i32), (qb["m12"], i32)):
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
    rows = np.full((pt_cap, 3), tl.FILL, f32)
    rows[:3] = pool["pos"][wa["pts"][:3]]
    for form in ("host", "batch"):
        assert take(i32).tolist() == [wa[k] for k in tl.SCALARS], form
        for k in ("win", "pts", "pts_kf"):
            assert take(i32).tolist() == wa[k], (form, k)
        assert np.array_equal(take(f32).reshape(pt_cap, 3), rows), form
        assert take(i32).tolist() == [wb[k] for k in tl.SCALARS] + [wb["num"]], form
        for k in ("win", "matched_mp", "matched_kf"):
            assert take(i32).tolist() == wb[k], (form, k)
    sb2 = plvi_lib.plvi_loop_window_scratch_bytes(2, len(pool["bad"]))
    assert take(i32).tolist() == [E_BADARG, E_BADARG, E_CAPACITY, E_BADARG, E_BADARG, sb2]
    assert pos == len(raw)
