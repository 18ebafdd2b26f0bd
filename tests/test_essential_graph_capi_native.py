"""A C++11 caller of plvi_loop_correct[_device] and plvi_essential_graph[_device]
(tests/native/essential_graph_capi_check.cpp) that includes only include/plvi_frontend.h, the way the INTEGRATION.md
shim of LoopClosing::CorrectLoop does: it compiles and links on the CPU host, the header's constants and struct sizes
are the Python mirror's, and on the GPU the host forms and the device forms both equal the host restatement
(tests/test_essential_graph.py) on a random map, C reading the stamps A left."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_essential_graph as te

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "essential_graph_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "essential_graph_capi_check"
NAMES = ("plvi_loop_correct", "plvi_loop_correct_device", "plvi_essential_graph", "plvi_essential_graph_device",
         "plvi_loop_connections_device", "plvi_loop_correct_scratch_bytes", "plvi_essential_graph_scratch_bytes")
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


def test_essential_graph_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout.split()
    for name in NAMES:
        assert name in out


def test_header_constants_and_struct_sizes_match_the_python_mirror():
    declared = set(plvi.exported_symbols())
    lib = plvi.load()
    for name in NAMES + ("plvi_loop_connections", "plvi_loop_connections_scratch_bytes", "plvi_covis_map_rows"):
        assert name in declared and getattr(lib, name).argtypes is not None
    got = subprocess.run([str(build()), "--sizes"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [plvi.EG_MAX_WIN, plvi.EG_MIN_FEAT, plvi.EG_4DOF, plvi.EG_EDGE_INERTIAL,
                                     plvi.EG_ERR_QUERY, plvi.EG_ERR_NO_VERTEX, plvi.EG_ERR_LC, plvi.COVIS_MAX_CONN,
                                     ctypes.sizeof(plvi.EgKeyframes), ctypes.sizeof(plvi.EgFeatures),
                                     ctypes.sizeof(plvi.LoopCorrectOutputs), ctypes.sizeof(plvi.EgOutputs)]
    assert plvi.EG_MAX_WIN == plvi.COVIS_MAX_CONN + 1      # the longest ordered row, and the keyframe itself


def test_scratch_bytes_contract():
    lib = plvi.load()
    a, c, b = (lib.plvi_loop_correct_scratch_bytes, lib.plvi_essential_graph_scratch_bytes,
               lib.plvi_loop_connections_scratch_bytes)
    assert a(-1, 1, 1) == 0 and a(1, -1, 1) == 0 and a(1, 1, -1) == 0
    assert a(64, 100, 300) == 256 + 1280            # a rank per slot, a position per id of the larger pool
    assert c(-1, 1, 1, 1) == 0 and c(1, 1, 1, -1) == 0
    assert c(64, 128, 10, 20) == 2 * 256 + 2 * 512 + 256
    assert b(-1, 1, 1) == 0 and b(3, 64, 32) == lib.plvi_covis_scratch_bytes(1, 64) + 256 + 2 * 256 + 512


@pytest.mark.gpu
def test_essential_graph_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    T, cur, loop, win, lc_kf, n_lc = te.random_case(3)
    mode = te.D7
    # one list of each call one entry short
    caps = dict(win_cap=T["C"] + 1, pt_cap=int(te.ref_correct(T, cur)["n_pts"][0]) - 1, ln_cap=len(T["lines"]["bad"]))
    gcaps = dict(vert_cap=T["K"], edge_cap=int(te.ref_graph(T, cur, loop, mode, win, lc_kf, n_lc)["n_edges"].sum()) - 1)
    exp_a = te.ref_correct(T, cur, **caps)
    stamps = {"points": (exp_a["pt_corr_by"], exp_a["pt_corr_ref"]), "lines": (exp_a["ln_corr_by"], exp_a["ln_corr_ref"])}
    exp_c = te.ref_graph(T, cur, loop, mode, win, lc_kf, n_lc, stamps, **gcaps)
    assert exp_a["err"][0] == te.E_PTS and exp_c["err"][0] & te.E_EDGE

    def blk(a, dt):
        b = np.ascontiguousarray(a, dt).tobytes()
        return np.array([len(b)], np.int32).tobytes() + b
    i32, u8, u32 = np.int32, np.uint8, np.uint32
    P, L = T["points"], T["lines"]
    blob = blk([T["K"], T["mp"].shape[1], T["ml"].shape[1], T["C"], len(T["order"]), len(P["bad"]), len(L["bad"]), cur,
                loop, mode, len(win), lc_kf.shape[1], caps["win_cap"], caps["pt_cap"], caps["ln_cap"],
                gcaps["vert_cap"], gcaps["edge_cap"]], i32)
    for k in te.KF_KEYS:
        blob += blk(T[k], T[k].dtype)
    for p in (P, L):
        for k, dt in (("bad", u8), ("ref_kf", i32), ("corr_by", u32), ("corr_ref", i32), ("map_id", i32)):
            blob += blk(p[k], dt)
    for a in (win, lc_kf, n_lc):
        blob += blk(a, i32)
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
        assert take().tolist() == [int(exp_a[k][0]) for k in ("n_win", "n_sorted", "n_pts", "n_lns", "err")], form
        for k in ("win", "win_sorted", "pts", "pts_kf", "lns", "lns_kf"):
            assert np.array_equal(take(), exp_a[k]), (form, k)
        for k, dt in (("pt_corr_by", u32), ("pt_corr_ref", i32), ("ln_corr_by", u32), ("ln_corr_ref", i32)):
            assert np.array_equal(take(dt), exp_a[k]), (form, k)
        assert take()[0] == (E_CAPACITY if form == "host" else 0), form
        assert take().tolist() == [int(exp_c["n_vert"][0]), int(exp_c["err"][0])], form
        for k in ("n_edges", "vert", "vert_flags", "edge_a", "edge_b", "edge_kind", "pt_ref", "ln_ref"):
            assert np.array_equal(take(), exp_c[k]), (form, k)
    sa = plvi_lib.plvi_loop_correct_scratch_bytes(T["K"], len(P["bad"]), len(L["bad"]))
    assert take().tolist() == [E_BADARG, E_BADARG, E_BADARG, E_CAPACITY, E_BADARG, E_CAPACITY, E_BADARG, sa]
    assert pos == len(raw)
