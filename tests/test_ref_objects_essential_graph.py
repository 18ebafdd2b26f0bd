"""Static pins on the reference's Optimizer.cc.o and LoopClosing.cc.o for the essential graph
(csrc/essential_graph.hip, tests/native/essential_graph_ref.cpp), read with objdump only.

Optimizer::OptimizeEssentialGraph(Map*, KeyFrame*, KeyFrame*, ..., LoopConnections, bFixScale) and
OptimizeEssentialGraph4DoF(Map*, ...):
* minFeat is one store of 100, the `int const&` handed to GetCovisiblesByWeight; `GetWeight(*sit) < minFeat` is a
  signed compare against 99 (cmp $0x63,%eax / jle) reached after two 64-bit mnId compares (the cur / loop
  exemption), in both functions;
* `pKFn->mnId < pKF->mnId` is an unsigned 64-bit compare (cmp %rcx,%rdx / jae: skip when not below), and stands
  right behind the second of the function's two KeyFrame::isBad() calls;
* those are the only two: the first guards the vertex loop (before GetRotation), the second is pKFn->isBad() behind
  hasChild.  Between the parent read (7DOF: GetParent; 4DoF: the loop-connection block) and GetLoopEdges there is
  none: the edge loop has no isBad() test on pKF;
* the 4DoF function calls neither GetParent nor Map::GetInitKFid (pParentKF is a literal NULL, the fixed vertex is
  pLoopKF), and tests the covisible against mPrevKF / mNextKF ahead of hasChild, which the 7DOF function does not;
* the point correction of the 4DoF function calls GetReferenceKeyFrame right behind isBad() with no compare between
  (mnCorrectedByKF is not read); the 7DOF function branches between the two.

LoopClosing::CorrectLoop / CorrectLoopWithLines: between GetConnectedKeyFrames and the optimiser call stand exactly two
set<KeyFrame*>::erase(key) call sites -- the previous neighbours and the window -- after a GetVectorCovisibleKeyFrames
and an UpdateConnections in that order (the snapshot is taken before the update).

Where these objects and the issue's reading disagree the object wins.  The module skips where the reference's build
tree is absent."""
import re
import subprocess

import pytest

from test_ref_objects import MAIN, pytestmark  # noqa: F401

O_OPT = MAIN / "src/Optimizer.cc.o"
O_LOOP = MAIN / "src/LoopClosing.cc.o"
EG7 = "ORB_SLAM3::Optimizer::OptimizeEssentialGraph(ORB_SLAM3::Map*, ORB_SLAM3::KeyFrame*, ORB_SLAM3::KeyFrame*,"
EG4 = "ORB_SLAM3::Optimizer::OptimizeEssentialGraph4DoF(ORB_SLAM3::Map*,"
_dump = {}


def ins(obj, prefix):
    """The instructions of the function whose demangled name starts with `prefix`, in address order as (address,
    text); a jump keeps its target address, a call is followed by ` [callee]`."""
    if obj not in _dump:
        _dump[obj] = subprocess.run(["objdump", "-dr", "--no-show-raw-insn", "-C", str(obj)], capture_output=True,
                                    text=True, check=True).stdout.splitlines()
    res, on = [], False
    for line in _dump[obj]:
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


BOTH = pytest.mark.parametrize("fn", [EG7, EG4], ids=["7dof", "4dof"])


@BOTH
def test_min_feat_is_100_and_the_weight_compare_is_signed(fn):
    code = ins(O_OPT, fn)
    stores = [t for _, t in code if re.fullmatch(r"movl \$0x64,-?0x[0-9a-f]+\(%r[bs]p\)", t)]
    assert len(stores) == 1, stores
    assert len(calls(code, "KeyFrame::GetCovisiblesByWeight(int const&)")) == 1
    w = calls(code, "KeyFrame::GetWeight(")
    assert len(w) == 1
    assert code[w[0] + 1][1] == "cmp $0x63,%eax" and code[w[0] + 2][1].startswith("jle ")
    assert not [t for _, t in code if re.fullmatch(r"cmpl? \$0x64,.*", t)]
    # the exemption: nIDi against pCurKF->mnId, nIDj against pLoopKF->mnId, 64-bit, ahead of the call
    before = [t for _, t in code[w[0] - 12:w[0]]]
    ids = [i for i, t in enumerate(before) if re.fullmatch(r"cmp 0x8\(%r\w+\),%r\w+", t)]
    assert len(ids) == 2 and before[ids[0] + 1].startswith("jne ") and before[ids[1] + 1].startswith("je ")


@BOTH
def test_mnid_compare_is_unsigned_and_follows_the_only_other_isbad(fn):
    code = ins(O_OPT, fn)
    bad = calls(code, "KeyFrame::isBad()")
    assert len(bad) == 2
    assert bad[0] < calls(code, "KeyFrame::GetRotation()")[0] < calls(code, "KeyFrame::GetWeight(")[0]
    child = calls(code, "KeyFrame::hasChild(")
    assert len(child) == 1 and child[0] < bad[1]
    after = [t for _, t in code[bad[1] + 1:bad[1] + 8]]
    assert after[0] == "test %al,%al" and after[1].startswith("jne ")
    assert re.fullmatch(r"mov 0x8\(%r\d+\),%rdx", after[2]) and re.fullmatch(r"mov 0x8\(%r\d+\),%rcx", after[3])
    assert after[4] == "cmp %rcx,%rdx" and after[5].startswith("jae ")
    # no isBad() on pKF in the edge loop
    loops = calls(code, "KeyFrame::GetLoopEdges()")
    assert len(loops) == 1 and not [i for i in bad if calls(code, "KeyFrame::GetWeight(")[0] < i < loops[0]]


def test_4dof_has_no_parent_branch_and_tests_prev_and_next():
    c7, c4 = ins(O_OPT, EG7), ins(O_OPT, EG4)
    assert len(calls(c7, "KeyFrame::GetParent()")) == 1 and not calls(c4, "KeyFrame::GetParent()")
    assert len(calls(c7, "Map::GetInitKFid()")) == 1 and not calls(c4, "Map::GetInitKFid()")
    chain = {}
    for name, code in (("7", c7), ("4", c4)):
        a, b = calls(code, "KeyFrame::GetCovisiblesByWeight(")[0], calls(code, "KeyFrame::hasChild(")[0]
        chain[name] = [t for _, t in code[a:b] if re.fullmatch(r"cmp 0x8[56][08]\(%r\d+\),%r\d+", t)]
    assert not chain["7"] and len(chain["4"]) >= 1, chain


def test_4dof_point_correction_reads_no_stamp():
    c7, c4 = ins(O_OPT, EG7), ins(O_OPT, EG4)
    for kind in ("MapPoint", "MapLine"):
        for name, code in (("7", c7), ("4", c4)):
            bad, ref = calls(code, kind + "::isBad()"), calls(code, kind + "::GetReferenceKeyFrame()")
            assert len(bad) == 1 and len(ref) == 1 and bad[0] < ref[0]
            between = [t for _, t in code[bad[0] + 1:ref[0]]]
            if name == "4":
                assert len(between) <= 4 and not [t for t in between if t.startswith("cmp")], between
            else:
                assert [t for t in between if t.startswith("cmp")] and len(between) > 4


@pytest.mark.parametrize("fn", ["CorrectLoop()", "CorrectLoopWithLines()"])
def test_loop_connections_has_two_erase_loops_behind_a_snapshot(fn):
    code = ins(O_LOOP, "ORB_SLAM3::LoopClosing::" + fn)
    conn = calls(code, "KeyFrame::GetConnectedKeyFrames()")
    opt = calls(code, "Optimizer::OptimizeEssentialGraph(")
    assert len(conn) == 1 and len(opt) == 1 and conn[0] < opt[0]
    erase = [i for i in calls(code, "::erase(ORB_SLAM3::KeyFrame* const&)") if "std::_Rb_tree<ORB_SLAM3::KeyFrame*, ORB_SLAM3::KeyFrame*," in code[i][1]]
    assert len(erase) == 2 and conn[0] < erase[0] < erase[1] < opt[0]
    snap = [i for i in calls(code, "KeyFrame::GetVectorCovisibleKeyFrames()") if i < conn[0]]
    upd = [i for i in calls(code, "KeyFrame::UpdateConnections(") if i < conn[0]]
    assert snap and upd and snap[-1] < upd[-1] < conn[0] and conn[0] - snap[-1] < 12
    assert len(calls(code, "Optimizer::OptimizeEssentialGraph4DoF(")) == 1
