"""Static pins on the reference's LocalMapping.cc.o for keyframe culling (csrc/cull.hip, tests/native/cull_ref.cpp),
read with objdump only, on KeyFrameCulling() and KeyFrameCullingWithLines():

* the redundancy test converts both ints to float, multiplies in float and compares in float (vcvtsi2ss / vmulss /
  vcomiss / jbe): no double product anywhere in either function;
* `cmp $0x3` / `jg` follows every Observations() call, of MapPoints and of MapLines;
* the point loop tests its observer count with `cmp $0x3` (jg to break, jle round the increment: strictly above 3),
  the line loop with `cmp $0x2` / `jg` (at least 3);
* KeyFramesInMap() is compared with `cmp $0x15` / `jbe`; mnId against the current keyframe's `sub $0x2` in 64 bits,
  unsigned (`ja`); last_ID is zero-extended from 32 bits before its 64-bit compare;
* t is a double subtraction narrowed at once (vsubsd, vcvtsd2ss) and compared as a float; the only double compares
  are the ones behind cv::norm;
* the break is `cmp $0x14` / `jle`, mbAbortBA, `cmp $0x64` / `jg`, and neither inertial `continue` reaches it
  without starting the next candidate;
* in the lines function the inertial branch calls KeyFrame::SetBadFlag() and the other one SetBadFlagWithLines(),
  and only the former lies behind a MergePrevious.

Where this object and the issue's reading disagree the object wins.  The module skips where
the reference's build tree is absent."""
import re
import subprocess

import pytest

from test_ref_objects import MAIN, pytestmark  # noqa: F401
from test_ref_objects_covis import _idx, _reach

O_LM = MAIN / "src/LocalMapping.cc.o"
FNS = ("KeyFrameCulling(", "KeyFrameCullingWithLines(")
_flows = {}


def _flow(fn):
    """The instructions of one function as (address, text, branch target or None), as test_ref_objects_covis._flow
    reads KeyFrame.cc.o."""
    prefix = "ORB_SLAM3::LocalMapping::" + fn
    if prefix in _flows:
        return _flows[prefix]
    out = subprocess.run(["objdump", "-dr", "--no-show-raw-insn", "-C", str(O_LM)], capture_output=True, text=True,
                         check=True).stdout
    res, on = [], False
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            on = m.group(1).startswith(prefix) and "[clone" not in m.group(1)
            continue
        if not on:
            continue
        m = re.match(r"^\s+[0-9a-f]+: (R_X86_64_\w+)\s+(.*)$", line)
        if m:
            sym = re.sub(r"[-+]0x[0-9a-f]+$", "", m.group(2)).strip()
            a, t, tg = res[-1]
            res[-1] = (a, t + " [" + re.sub(r"\(.*$", "", sym) + "]", None if t.startswith("call") else tg)
            continue
        m = re.match(r"^\s+([0-9a-f]+):\t(.*)$", line)
        if m:
            ins = re.sub(r"\s+#.*$", "", m.group(2)).strip()
            ins = re.sub(r"\s+<.*>$", "", ins)
            ins = re.sub(r"\s+", " ", ins)
            tg = re.match(r"^(call|j\w+) ([0-9a-f]+)$", ins)
            ins = re.sub(r"^(call|j\w+) [0-9a-f]+", r"\1", ins)
            res.append((int(m.group(1), 16), ins, int(tg.group(2), 16) if tg else None))
    assert res, prefix
    _flows[prefix] = res
    return res


def _ins(fn):
    return [t for _, t, _ in _flow(fn)]


def _after(ins, i, pat, gap=4):
    """The index of the first instruction matching `pat` within `gap` after i."""
    for j in range(i + 1, min(i + 1 + gap, len(ins))):
        if re.fullmatch(pat, ins[j]):
            return j
    raise AssertionError((ins[i:i + 1 + gap], pat))


@pytest.mark.parametrize("fn", FNS)
def test_redundancy_test_is_a_float_product_and_a_float_compare(fn):
    ins = _ins(fn)
    mul = [i for i, t in enumerate(ins) if t.startswith("vmulss")]
    assert len(mul) == (1 if fn == FNS[0] else 2)            # lines: nMPs + nMLs, and nMLs alone
    for i in mul:
        assert ins[i - 1].startswith("vcvtsi2ss")            # (float)n
        c = _after(ins, i, r"vcomiss %xmm\d+,%xmm\d+", 2)
        assert ins[c + 1] == "jbe"                           # not above: not redundant
    # (float)nRedundant is converted once more than there are products at most (the lines function reuses it)
    assert len(mul) + 1 <= len([t for t in ins if t.startswith("vcvtsi2ss")]) <= 2 * len(mul)
    assert not any(re.match(r"vmulsd|vcvtss2sd|vcvtsi2sd", t) for t in ins)


@pytest.mark.parametrize("fn", FNS)
def test_observations_must_exceed_three(fn):
    ins = _ins(fn)
    calls = [i for i, t in enumerate(ins) if re.fullmatch(r"call \[ORB_SLAM3::Map(Point|Line)::Observations\]", t)]
    assert len(calls) == (1 if fn == FNS[0] else 2)
    for i in calls:
        assert ins[i + 1] == "cmp $0x3,%eax" and ins[i + 2] == "jg"


def _loop_compares(ins, kind, nxt):
    """The compares of the observer count with a constant between the GetObservations call of `kind` and index nxt."""
    i = ins.index(f"call [ORB_SLAM3::Map{kind}::GetObservations]")
    return [(ins[j], ins[j + 1]) for j in range(i, nxt) if re.fullmatch(r"cmp \$0x[23],%r\d+d", ins[j])]


def test_points_need_four_other_observers_and_lines_three():
    for fn in FNS:
        ins = _ins(fn)
        nxt = ins.index("call [ORB_SLAM3::MapLine::GetObservations]") if fn == FNS[1] else len(ins)
        cmps = _loop_compares(ins, "Point", nxt)
        assert cmps and all(c.startswith("cmp $0x3,") for c, _ in cmps)            # nObs > thObs
        assert {j for _, j in cmps} == {"jg", "jle"}                               # the break, and round the ++
    ins = _ins(FNS[1])
    cmps = _loop_compares(ins, "Line", len(ins))
    assert cmps and all(c.startswith("cmp $0x2,") and j == "jg" for c, j in cmps)  # nObs >= thObs


@pytest.mark.parametrize("fn", FNS)
def test_inertial_gates(fn):
    flow, ins = _flow(fn), _ins(fn)
    at = {a: i for i, (a, _, _) in enumerate(flow)}
    gates = _idx(flow, "call [ORB_SLAM3::Atlas::KeyFramesInMap]")
    assert len(gates) == (1 if fn == FNS[0] else 2)
    body = _idx(flow, "call [ORB_SLAM3::KeyFrame::isBad]")
    assert len(body) == 1
    brk = [i for i, t in enumerate(ins) if re.fullmatch(r"cmp \$0x14,%\w+", t)]
    assert len(brk) == 1 and ins[brk[0] + 1] == "jle"                        # count > 20 ...
    b100 = _after(ins, brk[0], r"cmp \$0x64,%\w+", 6)
    assert ins[b100 + 1] == "jg" and any(t.startswith("cmpb $0x0,") for t in ins[brk[0]:b100])   # ... && mbAbortBA
    for g in gates:
        assert ins[g + 1] == "cmp $0x15,%rax" and ins[g + 2] == "jbe"        # KeyFramesInMap() <= Nd, unsigned
        s = _after(ins, g + 2, r"sub \$0x2,%r\w+", 5)
        assert re.fullmatch(r"cmp %r\w+,%r\w+", ins[s + 1]) and ins[s + 2] == "ja"   # 64-bit, unsigned
        for cont in (g + 2, s + 2):     # both `continue`s: the break test only after the next candidate's isBad
            assert brk[0] not in _reach(flow, at[flow[cont][2]], without=set(body))
        assert brk[0] in _reach(flow, cont + 1, without=set(body))           # the fall-through does reach it
        # t: a double subtraction narrowed at once
        sub = _after(ins, s + 2, r"vsubsd .*", 10)
        _after(ins, sub, r"vcvtsd2ss %xmm\d+,%xmm\d+,%xmm\d+", 2)
        # last_ID: a 32-bit load zero-extends, then a 64-bit compare
        ld = _after(ins, sub, r"mov 0x[0-9a-f]+\(%rsp\),%e\w+", 8)
        assert re.fullmatch(r"cmp %r\w+,%r\w+", ins[ld + 1]) and ins[ld + 2] in ("jae", "jb")
    dbl = [i for i, t in enumerate(ins) if t.startswith(("vcomisd", "vucomisd"))]
    norm = _idx(flow, "call [cv::norm]")
    assert len(dbl) == len(norm) == len(gates)
    for n in norm:
        _after(ins, n, r"vcomisd .*", 3)                                     # norm < 0.02, the one double compare
    assert len([t for t in ins if t.startswith("vsubsd")]) == len(gates)


def test_lines_function_erases_lines_only_outside_the_inertial_branch():
    flow = _flow(FNS[1])
    plain = _idx(flow, "call [ORB_SLAM3::KeyFrame::SetBadFlag]")
    with_lines = _idx(flow, "call [ORB_SLAM3::KeyFrame::SetBadFlagWithLines]")
    merge = _idx(flow, "call [ORB_SLAM3::IMU::Preintegrated::MergePrevious]")
    assert plain and with_lines and merge
    for m in merge:      # a relink is followed by SetBadFlag() and never by SetBadFlagWithLines()
        seen = _reach(flow, m + 1, without=set(plain) | set(_idx(flow, "call [ORB_SLAM3::KeyFrame::isBad]")))
        assert not seen & set(with_lines)
        assert _reach(flow, m + 1, without=set(_idx(flow, "call [ORB_SLAM3::KeyFrame::isBad]"))) & set(plain)
    flow0 = _flow(FNS[0])
    assert _idx(flow0, "call [ORB_SLAM3::KeyFrame::SetBadFlag]")
    assert not _idx(flow0, "call [ORB_SLAM3::KeyFrame::SetBadFlagWithLines]")
