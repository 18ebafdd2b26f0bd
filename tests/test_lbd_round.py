"""The LBD sample-coordinate rounding of lbd_describe_kernel
(plvi_round_clamp_i16, csrc/plvi_math.h) equals the reference's
(short)roundf + clamp for every float the cast is defined for."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "lbd_round_check.cpp"
BIN = ROOT / "tests" / "native" / "_build" / "lbd_round_check"


def test_round_clamp_every_float():
    BIN.parent.mkdir(exist_ok=True)
    hdr = ROOT / "pl-vi-orbslam3_amd" / "csrc" / "plvi_math.h"
    if not BIN.exists() or BIN.stat().st_mtime < max(SRC.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-o", str(BIN),
                        str(SRC), "-lm"], check=True)
    r = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mismatches=0" in r.stdout, r.stdout + r.stderr
    # both signs: every float below 32767.5 in magnitude, and -32768 .. -32767.5
    n = int(r.stdout.split("checked=")[1].split()[0])
    assert n > 2 * 0x46FFFF00
