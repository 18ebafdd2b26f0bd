"""Static pins on the reference's LoopClosing.cc.o for the loop-detection windows (csrc/loop_window.hip,
tests/native/loop_window_ref.cpp), read with objdump only.

LoopClosing::FindMatchesByProjection (not inlined: DetectAndReffineSim3FromLastKF calls it twice,
DetectCommonRegionsFromLastKF once):
* nNumCovisibles is one store of 5; GetBestCovisibilityKeyFrames has two call sites (pMatchedKFw's, and the one in
  the loop over the first nInitialCov members) and GetConnectedKeyFrames one;
* `nInserted < nNumCovisibles` is a signed compare (cmp / jle) whose exit, like the exit of `j < vpKFs.size()`
  (unsigned, ja on the way back), lands on the block that calls vector::_M_range_insert: between that landing and
  the call there is no branch.  The range insert of :1181 is not guarded by the nInserted loop: every row is
  appended whole.

LoopClosing::DetectCommonRegionsFromBoW:
* nNumCovisibles = 5 (one store, handed to three GetBestCovisibilityKeyFrames call sites: :802, :893 and the
  bounding-box block), one GetConnectedKeyFrames call site;
* numBoWMatches >= 20, numOptMatches >= 20, numProjMatches >= 50 and numProjOptMatches >= 80 are signed compares
  against 19, 19, 49 (jle) and 79 (jg); solver.iterate takes 20.

LoopClosing::DetectAndReffineSim3FromLastKF: nProjMatches = 30 (cmp 29 / jle), numOptMatches > 50 (cmp 50 / jle),
numProjOptMatches >= 100 (cmp 99 / jg), all signed; DetectCommonRegionsFromLastKF compares against 29 too.

The thresholds stay with the caller; they are pinned here because INTEGRATION.md's call order names them.  Where
this object and the issue's reading disagree the object wins.  The module skips where the reference's build tree is
absent."""
import re
import subprocess

import pytest

from test_ref_objects import MAIN, pytestmark  # noqa: F401

O_LOOP = MAIN / "src/LoopClosing.cc.o"
FMBP = "FindMatchesByProjection("
BOW = "DetectCommonRegionsFromBoW("
REFF = "DetectAndReffineSim3FromLastKF("
LASTKF = "DetectCommonRegionsFromLastKF("
_dump = {}


def ins(fn):
    """The instructions of LoopClosing::<fn> in address order as (address, text); a jump keeps its target address,
    a call is followed by ` [callee]`."""
    if not _dump:
        _dump["txt"] = subprocess.run(["objdump", "-dr", "--no-show-raw-insn", "-C", str(O_LOOP)], capture_output=True,
                                      text=True, check=True).stdout.splitlines()
    prefix = "ORB_SLAM3::LoopClosing::" + fn
    res, on = [], False
    for line in _dump["txt"]:
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            on = m.group(1).startswith(prefix) and "[clone" not in m.group(1)
            continue
        if not on:
            continue
        m = re.match(r"^\s+[0-9a-f]+: R_X86_64_\w+\s+(.*)$", line)
        if m and res:
            callee = re.sub(r"[-+]0x[0-9a-f]+$", "", m.group(1)).strip()
            res[-1] = (res[-1][0], res[-1][1] + " [" + callee + "]")
            continue
        m = re.match(r"^\s+([0-9a-f]+):\t(.*)$", line)
        if m:
            t = re.sub(r"\s+<.*>$", "", re.sub(r"\s+#.*$", "", m.group(2)).strip())
            t = re.sub(r"^call [0-9a-f]+$", "call", re.sub(r"\s+", " ", t))
            res.append((int(m.group(1), 16), t))
    assert res, prefix
    return res


def calls(code, name):
    return [i for i, (_, t) in enumerate(code) if t.startswith("call") and name in t]


def compares(code, imm):
    """The branch that follows each compare against the immediate."""
    return [code[i + 1][1].split()[0] for i, (_, t) in enumerate(code)
            if re.fullmatch(rf"cmpl? \${imm:#x},.*", t)]


def test_find_matches_by_projection_call_sites():
    code = ins(FMBP)
    assert len(calls(code, "KeyFrame::GetBestCovisibilityKeyFrames(")) == 2
    assert len(calls(code, "KeyFrame::GetConnectedKeyFrames(")) == 1
    assert len(calls(code, "_M_range_insert<")) == 1
    stores = [t for _, t in code if re.fullmatch(r"movl \$0x5,-0x[0-9a-f]+\(%rbp\)", t)]
    assert len(stores) == 1, stores
    # it stands alone: its callers call it, and the validation loop of DetectCommonRegionsFromBoW reaches it
    # through its one call of DetectCommonRegionsFromLastKF
    for fn, n in ((REFF, 2), (LASTKF, 1), (BOW, 0)):
        assert len(calls(ins(fn), "LoopClosing::FindMatchesByProjection(")) == n, fn
    assert len(calls(ins(BOW), "LoopClosing::DetectCommonRegionsFromLastKF(")) == 1


def test_range_insert_is_not_guarded_by_the_ninserted_loop():
    code = ins(FMBP)
    slot = [t for _, t in code if re.fullmatch(r"movl \$0x5,-0x[0-9a-f]+\(%rbp\)", t)][0].split(",")[1]
    second = calls(code, "KeyFrame::GetBestCovisibilityKeyFrames(")[1]
    insert = calls(code, "_M_range_insert<")[0]
    unique = [i for i in calls(code, "_M_insert_unique<") if second < i < insert]
    assert len(unique) == 1                          # spCheckKFs.insert inside the while loop
    body = code[second:insert]
    # `nInserted < nNumCovisibles`: signed, the count against the stored 5
    test = [i for i, (_, t) in enumerate(body) if re.fullmatch(rf"cmp %r\d+d,{re.escape(slot)}", t)]
    assert len(test) == 1 and body[test[0] + 1][1].startswith("jle ")
    exit_to = int(body[test[0] + 1][1].split()[1], 16)
    # `j < vpKFs.size()`: unsigned, the last branch before the range insert, back into the loop
    back = max(i for i, (_, t) in enumerate(body) if re.match(r"j\w+ ", t))
    assert body[back][1].startswith("ja ") and int(body[back][1].split()[1], 16) == body[test[0]][0]
    # both exits land right behind it, and from there to the call nothing branches
    assert body[back + 1][0] == exit_to
    tail = [t for _, t in body[back + 1:]]
    assert tail and all(re.match(r"(mov|lea) ", t) for t in tail), tail
    # an empty row takes the same way
    empty = [t for _, t in body if t.startswith("je ") and int(t.split()[1], 16) == exit_to]
    assert len(empty) == 1


def test_bow_window_constants_and_call_sites():
    code = ins(BOW)
    assert len(calls(code, "KeyFrame::GetBestCovisibilityKeyFrames(")) == 3
    assert len(calls(code, "KeyFrame::GetConnectedKeyFrames(")) == 1
    assert len([t for _, t in code if re.fullmatch(r"movl \$0x5,-0x[0-9a-f]+\(%rbp\)", t)]) == 1
    assert compares(code, 19) == ["jle", "jle"]      # numBoWMatches >= 20, numOptMatches >= 20
    assert compares(code, 49) == ["jle"]             # numProjMatches >= 50
    assert compares(code, 79) == ["jg"]              # numProjOptMatches >= 80
    assert not compares(code, 20) and not compares(code, 50) and not compares(code, 80)
    it = calls(code, "Sim3Solver::iterate(")
    assert len(it) == 1 and "mov $0x14,%edx" in [t for _, t in code[it[0] - 12:it[0]]]


def test_last_kf_thresholds():
    code = ins(REFF)
    assert compares(code, 29) == ["jle"]             # numProjMatches >= 30
    assert compares(code, 50) == ["jle"]             # numOptMatches > 50
    assert compares(code, 99) == ["jg"]              # numProjOptMatches >= 100
    assert not compares(code, 30) and not compares(code, 100)
    last = ins(LASTKF)
    at = [i for i, (_, t) in enumerate(last) if re.fullmatch(r"cmp \$0x1d,%eax", t)]
    assert len(at) == 1
    assert [t.split()[0] for _, t in last[at[0] + 1:at[0] + 6] if re.match(r"(set|cmov|j)", t)][0] in ("setg", "jg", "jle")
