"""The ORB pyramid kernels' packed column table (csrc/orb_xtab.h) on the host:
tests/native/xtab_check.cpp builds it with the product's append_xtab and
re-derives cv::resize's sx / a0 / a1 for every (source width, level width)
pair that tests/test_orb_pyramid_quads_gpu.py and the default configuration
use, plus the padding, the wide-level flag and the 8-byte tap window."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "xtab_check.cpp"
BIN = ROOT / "tests" / "native" / "_build" / "xtab_check"
CSRC = ROOT / "pl-vi-orbslam3_amd" / "csrc"

# source:level[:a] -- the chained level widths of the GPU test's cases and of 640 / 752 x 480, scale 1.2, 8 levels
PAIRS = ["307:256", "256:213", "308:257", "257:214", "614:512", "616:513", "1024:853", "853:711", "74:62",
         "320:267", "267:222", "222:185", "185:154", "154:129", "129:107", "107:89",
         "300:286", "286:272", "272:259", "322:161:a", "200:100:a", "322:161", "400:160",
         "640:533", "533:444", "444:370", "370:309", "309:257", "257:214", "214:179",
         "752:627", "627:522", "522:435", "435:363", "363:302", "302:252", "252:210"]
WIDE = {"400:160"}


def test_xtab_matches_cv_resize_columns():
    BIN.parent.mkdir(exist_ok=True)
    hdr = CSRC / "orb_xtab.h"
    if not BIN.exists() or BIN.stat().st_mtime < max(SRC.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", f"-I{CSRC}",
                        f"-I{ROOT / 'include'}", "-o", str(BIN), str(SRC), "-lm"], check=True)
    r = subprocess.run([str(BIN), *PAIRS], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches=0" in r.stdout
    n = sum((int(p.split(":")[1]) + 3) & ~3 for p in PAIRS)
    assert f"checked={n} " in r.stdout


def test_xtab_wide_levels_are_flagged():
    """Scale 2.5 (400 -> 160): a quad's taps span more than 8 bytes, so the level is flagged; the 1.2,
    1.05 and 2.0 levels are not (the check above proves their taps fit the window)."""
    test_xtab_matches_cv_resize_columns()
    for p in ("400:160", "640:533", "322:161", "300:286"):
        r = subprocess.run([str(BIN), p], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
    src = (CSRC / "orb_xtab.h").read_text()
    assert "kPyrXtabWide = 1u << 26" in src
