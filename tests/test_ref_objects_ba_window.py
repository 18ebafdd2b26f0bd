"""Static pins on the reference's Optimizer.cc.o for the local-BA window (csrc/ba_window.hip,
tests/native/ba_window_ref.cpp), read with objdump only.

Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*, int&):
* `pKFi->mnId < lowerId` and `pKFi->mnId < secondLowerId` load the 64-bit mnId, SIGN-extend the int (movslq) and
  branch unsigned (jb / jae): an int made negative by a large mnId is above every id.  The restatement writes the
  compare as the reference does and the kernel spells out the sign extension;
* both `num_fixedKF < 2` tests are `cmp $0x1` / `jle`: signed, against 1.

Optimizer::LocalInertialBA:
* maxOpt is 25 - 15 * !bLarge (sbb / and $0xfffffff1 / add $0x19), Nd is KeyFramesInMap() - 2 in 32 bits (lea -0x2)
  and a signed min (cmovg);
* `lFixedKeyFrames.size() >= maxFixKF` is `cmp $0xc7` / `ja` on the 64-bit size: unsigned, above 199;
* GetMapPointMatches() is called at one site only: the covisible loop of :9255 (maxCovKF = 0) kept none.

Optimizer::LocalBundleAdjustmentOnlyLines: between the first KeyFrame::isBad() and GetMapLineMatches() there is no
GetMap() call -- the lines function lists covisibles of other maps -- while the points function has one between its
first isBad() and GetMapPointMatches().

Where this object and the issue's reading disagree the object wins.  The module skips where the reference's build
tree is absent."""
import re
import subprocess

import pytest

from test_ref_objects import MAIN, pytestmark  # noqa: F401

O_OPT = MAIN / "src/Optimizer.cc.o"
LBA = "LocalBundleAdjustment(ORB_SLAM3::KeyFrame*, bool*, ORB_SLAM3::Map*, int&)"
LINES = "LocalBundleAdjustmentOnlyLines(ORB_SLAM3::KeyFrame*, bool*, ORB_SLAM3::Map*)"
INERTIAL = "LocalInertialBA("
_dump = {}


def ins(fn):
    """The instructions of Optimizer::<fn> in address order, a call followed by ` [callee]`."""
    if not _dump:
        _dump["txt"] = subprocess.run(["objdump", "-dr", "--no-show-raw-insn", "-C", str(O_OPT)], capture_output=True,
                                      text=True, check=True).stdout.splitlines()
    prefix = "ORB_SLAM3::Optimizer::" + fn
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
            res[-1] += " [" + re.sub(r"\(.*$", "", re.sub(r"[-+]0x[0-9a-f]+$", "", m.group(1)).strip()) + "]"
            continue
        m = re.match(r"^\s+[0-9a-f]+:\t(.*)$", line)
        if m:
            t = re.sub(r"\s+<.*>$", "", re.sub(r"\s+#.*$", "", m.group(1)).strip())
            res.append(re.sub(r"^(call|j\w+) [0-9a-f]+$", r"\1", re.sub(r"\s+", " ", t)))
    assert res, prefix
    return res


def after(code, i, pat, gap=3):
    for j in range(i + 1, min(i + 1 + gap, len(code))):
        if re.fullmatch(pat, code[j]):
            return j
    raise AssertionError((code[i:i + 1 + gap], pat))


def test_lower_id_is_sign_extended_and_compared_unsigned():
    code = ins(LBA)
    ext = [i for i, t in enumerate(code) if re.fullmatch(r"movslq %r\d+d,%r\w+", t)]
    pairs = []
    for i in ext:
        reg = code[i].split(",")[1]
        if i + 2 < len(code) and re.fullmatch(rf"cmp {re.escape(reg)},%r\w+", code[i + 1]) and \
                re.fullmatch(r"j(b|ae)", code[i + 2]):
            pairs.append(code[i + 2])
    assert pairs == ["jb", "jae"], pairs      # `if (<) ... else if (<)`: taken below, left at or above
    # the other operand is the 64-bit mnId, loaded just before
    i = [j for j in ext if code[j + 2] == "jb"][0]
    assert re.fullmatch(r"mov 0x8\(%r\w+\),%rax", code[i - 1]) and code[i + 1].endswith(",%rax")


def test_num_fixed_below_two_is_signed_against_one():
    code = ins(LBA)
    at = [i for i, t in enumerate(code) if t == "cmp $0x1,%eax"]
    assert len(at) == 2 and all(code[i + 1] == "jle" for i in at)
    assert code[at[1] - 2] == "add $0x1,%eax", "the second test follows num_fixedKF++"


def test_inertial_window_size():
    code = ins(INERTIAL)
    i = code.index("add $0x19,%ebx")
    assert code[i - 1] == "and $0xfffffff1,%ebx" and "sbb %ebx,%ebx" in code[i - 5:i]    # 25, or 25 - 15
    k = [j for j, t in enumerate(code) if t.startswith("call") and t.endswith("[ORB_SLAM3::Map::KeyFramesInMap]")]
    assert len(k) == 1
    j = after(code, k[0], r"lea -0x2\(%rax\),%r\d+d", 6)
    reg = code[j].split(",")[1]
    c = after(code, j, rf"cmp %ebx,{reg}", 4)
    after(code, c, rf"cmovg %ebx,{reg}", 6)


def test_inertial_cap_is_unsigned_above_199():
    code = ins(INERTIAL)
    at = [i for i, t in enumerate(code) if re.fullmatch(r"cmp \$0xc7,%r\w+", t)]
    assert len(at) == 1 and code[at[0] + 1] == "ja"
    assert not [t for t in code if re.search(r"\$0xc8\b", t)]


def test_inertial_covisible_loop_kept_no_table_read():
    code = ins(INERTIAL)
    calls = [t for t in code if t.startswith("call") and "GetMapPointMatches" in t]
    assert len(calls) == 1, calls


def _between(code, first, last):
    a = next(i for i, t in enumerate(code) if t.startswith("call") and t.endswith(f"[{first}]"))
    b = next(i for i, t in enumerate(code) if i > a and t.startswith("call") and t.endswith(f"[{last}]"))
    return [t for t in code[a:b] if t.startswith("call")]


def test_lines_function_has_no_map_test_on_its_covisibles():
    lines = _between(ins(LINES), "ORB_SLAM3::KeyFrame::isBad", "ORB_SLAM3::KeyFrame::GetMapLineMatches")
    assert not [t for t in lines if "KeyFrame::GetMap]" in t], lines
    points = _between(ins(LBA), "ORB_SLAM3::KeyFrame::isBad", "ORB_SLAM3::KeyFrame::GetMapPointMatches")
    assert [t for t in points if "KeyFrame::GetMap]" in t], points
