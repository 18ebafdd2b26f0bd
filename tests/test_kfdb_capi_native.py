"""A C++11 caller of the plvi_kfdb_* entry points (tests/native/kfdb_capi_check.cpp) that includes only
include/plvi_frontend.h, the way the INTEGRATION.md shims of Tracking::Relocalization and
LoopClosing::NewDetectCommonRegions do: it compiles and links on the CPU host, and on the GPU its results equal the
host restatement's (tests/test_kfdb.py)."""
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_kfdb as tk

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "kfdb_capi_check.cpp"
EXE = ROOT / "tests" / "native" / "_build" / "kfdb_capi_check"
NAMES = ("plvi_kfdb_create", "plvi_kfdb_destroy", "plvi_kfdb_add", "plvi_kfdb_add_batch", "plvi_kfdb_errors",
         "plvi_kfdb_query", "plvi_kfdb_query_batch")


def build():
    if EXE.exists() and EXE.stat().st_mtime > max(SRC.stat().st_mtime, plvi.LIB_PATH.stat().st_mtime,
                                                    plvi.HEADER_PATH.stat().st_mtime):
        return EXE
    EXE.parent.mkdir(parents=True, exist_ok=True)
    libdir = plvi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o",
                    str(EXE), f"-L{libdir}", "-lplvi_frontend", f"-Wl,-rpath,{libdir}"], check=True)
    return EXE


def test_kfdb_capi_check_compiles_and_links():
    exe = build()
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True).stdout.split()
    for name in NAMES:
        assert name in out


def test_header_limits_match_the_python_mirror():
    txt = plvi.HEADER_PATH.read_text()
    assert f"#define PLVI_KFDB_MAX_WORDS {plvi.KFDB_MAX_WORDS} " in txt
    assert f"#define PLVI_KFDB_NEIGHBOURS {plvi.KFDB_NEIGHBOURS} " in txt
    assert plvi.KFDB_MAX_WORDS >= 5000  # the initial keyframes' 5 * nFeatures extractor (Tracking.cc:921)
    assert 12 * plvi.KFDB_MAX_WORDS <= 160 * 1024  # the staged query fits a CU's LDS
    declared = set(plvi.exported_symbols())
    for name in NAMES + ("plvi_kfdb_erase", "plvi_kfdb_clear_map", "plvi_kfdb_clear"):
        assert name in declared


@pytest.mark.gpu
def test_kfdb_capi_check_matches_restatement(plvi_lib, tmp_path):
    exe = build()
    case = tk.general_case()
    adds = case.ops[0][1][:60]
    q = case.ops[-1][1]  # the mode 1 query op: bows, maps, connected, covis, bad
    nq = len(q["bows"])
    i32 = lambda *x: np.array(x, np.int32).tobytes()  # noqa: E731
    blob = i32(case.n_words, case.slot_cap, case.word_cap, len(adds), nq, len(q["bad"]))
    for slot, (w, v), m in adds:
        blob += i32(slot, m, len(w)) + w.tobytes() + v.tobytes()
    for (w, v), m, conn in zip(q["bows"], q["maps"], q["connected"]):
        blob += i32(m, len(w), len(conn)) + w.tobytes() + v.tobytes() + i32(*sorted(conn))
    blob += q["covis"].tobytes() + np.array(q["bad"], np.uint8).tobytes()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=120)

    # the same sequence on the restatement: per query a mode 0 and a mode 1 call, then one batch per mode
    ref = tk.Case(case.n_words, case.slot_cap, case.word_cap)
    ref.add(*adds)
    for i in range(nq):
        ref.query(q["bows"][i:i + 1], q["maps"][i:i + 1], 0, covis=q["covis"])
        ref.query(q["bows"][i:i + 1], q["maps"][i:i + 1], 1, connected=q["connected"][i:i + 1], covis=q["covis"],
                  bad=q["bad"])
    ref.query(q["bows"], q["maps"], 0, covis=q["covis"])
    ref.query(q["bows"], q["maps"], 1, connected=q["connected"], covis=q["covis"], bad=q["bad"])
    exp = tk.run_host(ref, tk.RefDB)[0]
    assert sum(len(e["a"]) for e in exp) >= 20 and sum(len(e["b"]) for e in exp) >= 10

    words = np.frombuffer(dst.read_bytes(), np.int32).tolist()
    pos = 0

    def take(n):
        nonlocal pos
        pos += n
        return words[pos - n:pos]

    for i in range(nq):
        e0, e1 = exp[2 * i], exp[2 * i + 1]
        assert take(1) == [len(e0["a"])] and take(len(e0["a"])) == e0["a"]
        assert take(1) == [len(e1["a"])] and take(len(e1["a"])) == e1["a"]
        assert take(1) == [len(e1["b"])] and take(len(e1["b"])) == e1["b"]
    b0, b1 = exp[2 * nq:3 * nq], exp[3 * nq:]

    def rows(lists):
        return [x for lst in lists for x in (lst[:3] + [-7] * 3)[:3]]

    assert take(nq) == [len(e["a"]) for e in b0]          # the full count, three candidates a row kept
    assert take(3 * nq) == rows([e["a"] for e in b0])
    assert take(nq) == [len(e["a"]) for e in b1] and take(3 * nq) == rows([e["a"] for e in b1])
    assert take(nq) == [len(e["b"]) for e in b1] and take(3 * nq) == rows([e["b"] for e in b1])
    assert take(5) == [tk.E_BADARG, tk.E_BADARG, tk.E_BADARG, tk.E_CAPACITY, 0]
    assert pos == len(words)
