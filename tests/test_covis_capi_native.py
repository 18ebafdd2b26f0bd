"""A C++11 caller of the plvi_covis_* entry points (tests/native/covis_capi_check.cpp) that includes only
include/plvi_frontend.h, the way the INTEGRATION.md shims of KeyFrame::UpdateConnections do: it compiles and links on
the CPU host, the header's constants and struct sizes are the Python mirror's, and on the GPU the host form and the
batch form both equal the host restatement (tests/test_covis.py) on a random map with lines."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_covis as tc

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "covis_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "covis_capi_check"
NAMES = ("plvi_covis_create", "plvi_covis_destroy", "plvi_covis_scratch_bytes", "plvi_covis_update_batch",
         "plvi_covis_update", "plvi_covis_download", "plvi_covis_weight_batch", "plvi_covis_by_weight_batch")
ALL = NAMES + ("plvi_covis_erase_batch", "plvi_covis_resort_batch", "plvi_covis_rows")


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_covis_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout.split()
    for name in NAMES:
        assert name in out


def test_header_constants_and_struct_sizes_match_the_python_mirror():
    txt = plvi.HEADER_PATH.read_text()
    assert f"#define PLVI_COVIS_LDS_KF {plvi.COVIS_LDS_KF} " in txt
    assert f"#define PLVI_COVIS_MAX_CONN {plvi.COVIS_MAX_CONN} " in txt
    assert f"#define PLVI_COVIS_TH {plvi.COVIS_TH} " in txt
    assert f"#define PLVI_COVIS_MAX_QUERIES {plvi.COVIS_MAX_QUERIES}\n" in txt
    declared = set(plvi.exported_symbols())
    lib = plvi.load()
    for name in ALL:
        assert name in declared and getattr(lib, name).argtypes is not None
    # what the C compiler makes of the header (the program prints it without touching a device)
    got = subprocess.run([str(build()), "--sizes"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [plvi.COVIS_LDS_KF, plvi.COVIS_MAX_CONN, plvi.COVIS_TH, plvi.COVIS_MAX_QUERIES,
                                     ctypes.sizeof(plvi.CovisKeyframes), ctypes.sizeof(plvi.CovisOutputs)]
    assert ctypes.sizeof(plvi.CovisKeyframes) == 16 + 11 * 8 and ctypes.sizeof(plvi.CovisOutputs) == 6 * 8
    # the count kernel's LDS: the histogram (4 B a slot), the sort keys and slots (12 B an entry) inside 64 KB
    assert plvi.COVIS_LDS_KF * 4 + plvi.COVIS_MAX_CONN * 12 <= 60 * 1024


@pytest.mark.gpu
def test_covis_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    m, _, _ = tc.random_case(2003, K=20, kp_cap=400)
    assert m.kl_cap and m.map_id is None
    q = np.random.default_rng(3).permutation(m.K).astype(np.int32)
    ref = tc.RefRunner(m).run([("update", q.tolist())])
    assert max(ref[0]["n_conn"]) > 3 and any(p >= 0 for p in ref[0]["new_parent"])
    kf, mp, ml = m.ctables()

    def blk(a, dt):
        b = np.ascontiguousarray(a, dt).tobytes()
        return np.array([len(b)], np.int32).tobytes() + b
    i32, u8 = np.int32, np.uint8
    blob = blk([m.K, len(kf["order"]), m.kp_cap, m.kl_cap, len(mp["bad"]), len(ml["bad"]), m.conn_cap, len(q)], i32)
    for a, dt in ((kf["bad"], u8), (kf["order"], i32), (kf["mp"], i32), (kf["nmp"], i32), (kf["ml"], i32),
                  (kf["nml"], i32), (m.init, u8), (m.first, u8), (m.parent, i32), (mp["bad"], u8),
                  (mp["obs_off"], i32), (mp["obs_kf"], i32), (ml["bad"], u8), (ml["obs_off"], i32),
                  (ml["obs_kf"], i32), (q, i32)):
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
    want = np.array([ref[0][k] for k in tc.OUTS], np.int32).T
    for form in ("host", "batch"):
        assert np.array_equal(take(i32).reshape(-1, 6), want), form
        assert take(u8).tolist() == ref[-1]["first"], form
        assert take(i32).tolist() == ref[-1]["parent"], form
        assert take(i32).reshape(-1, 10).tolist() == ref[-1]["covis"], form
        for s in range(m.K):
            wm, wo = ref[-1]["state"][s]
            assert take(i32).tolist() == [len(wm), len(wo), 0], (form, s)
            assert take(i32).tolist() == [k for k, _ in wm] and take(i32).tolist() == [w for _, w in wm], (form, s)
            assert take(i32).tolist() == [k for k, _ in wo] and take(i32).tolist() == [w for _, w in wo], (form, s)
    w01 = dict(map(tuple, ref[-1]["state"][int(q[0])][0])).get(int(q[1]), 0)
    n15 = sum(1 for _, w in ref[-1]["state"][int(q[0])][1] if w >= 15)
    assert take(i32).tolist() == [tc.E_BADARG, tc.E_BADARG, 0, tc.E_CAPACITY, w01, n15]
    assert pos == len(raw)
