"""Static pins on the reference's LoopClosing.cc.o for the GBA propagation (csrc/gba_propagate.hip,
tests/native/gba_propagate_ref.cpp), read with objdump only.

LoopClosing::RunGlobalBundleAdjustment(unsigned long) and RunGlobalBundleAdjustmentWithLines(unsigned long):
* the child loop has the function's single KeyFrame::isBad() call, behind the NULL test of the set's entry; right
  behind it stands the compare of the child's mnBAGlobalForKF (a 64-bit member at 0x238) with nLoopKF.  Equal jumps
  straight to the push_back (operator new(0x18) + _List_node_base::_M_hook, the only one behind GetChilds); unequal
  falls into the pose block (GetPose, four operator*) and runs into the same push_back: a child is queued whether
  it is new or not.  NULL and bad jump past it, to _Rb_tree_increment;
* the front entry is tested for nothing: between the read of the list's front and GetChilds / GetPoseInverse there
  is no call and no compare, and GetPose / SetPose follow the child loop unconditionally;
* each feature loop is isBad(), the compare of the feature's mnBAGlobalForKF with nLoopKF (SetWorldPos(mPosGBA) on
  equal), GetReferenceKeyFrame(), the compare of the keyframe's stamp at 0x238, then cv::Mat::empty() on
  mTcwBefGBA at 0x100 -- and no KeyFrame::isBad() on the reference keyframe;
* the product sites are operator*(Mat const&, Mat const&) followed by operator+(MatExpr const&, Mat const&), the
  pair Frame.cc.o shows for Rcw * P + tcw in Frame::isInFrustum: two pairs per MapPoint, four per MapLine, the
  second half behind GetPoseInverse(), the line results through Converter::toVector3d;
* neither function has a fused multiply-add of its own.

The stamps are 64-bit in the object; the tables carry them as `unsigned`, like kf_id.  Where these objects and the
issue's reading disagree the object wins; they do not.  The module skips where the reference's build tree is
absent."""
import re

import pytest

from test_ref_objects import FMA, MAIN, pytestmark  # noqa: F401
from test_ref_objects_essential_graph import O_LOOP, calls, ins

FNS = ["ORB_SLAM3::LoopClosing::RunGlobalBundleAdjustment(", "ORB_SLAM3::LoopClosing::RunGlobalBundleAdjustmentWithLines("]
BOTH = pytest.mark.parametrize("fn", FNS, ids=["points-object", "lines-object"])
MUL, ADD = "cv::operator*(cv::Mat const&, cv::Mat const&)", "cv::operator+(cv::MatExpr const&, cv::Mat const&)"
STAMP = r"cmp %r\w+,0x238\(%r\w+\)"


def at(code, address):
    return next(i for i, (a, _) in enumerate(code) if a == address)


def target(text):
    return int(text.split()[1], 16)


@BOTH
def test_child_loop_one_isbad_then_the_stamp_and_push_back_on_both_sides(fn):
    code = ins(O_LOOP, fn)
    bad = calls(code, "KeyFrame::isBad()")
    assert len(bad) == 1
    b = bad[0]
    childs, inc = calls(code, "KeyFrame::GetChilds()"), calls(code, "_Rb_tree_increment")
    assert len(childs) == 1 and childs[0] < b
    # the NULL test ahead of it and the bad test behind it leave for the same place: the increment
    assert re.fullmatch(r"test %r\w+,%r\w+", code[b - 3][1]) and code[b - 2][1].startswith("je ")
    assert code[b + 1][1] == "test %al,%al" and code[b + 2][1].startswith("jne ")
    skip = target(code[b + 2][1])
    assert target(code[b - 2][1]) == skip
    nxt = [i for i in inc if code[i][0] > skip][0]
    assert at(code, skip) == nxt - 1
    # the stamp compare, 64-bit, and where its two sides go
    assert re.fullmatch(r"mov -?0x[0-9a-f]+\(%r[bs]p\),%rax", code[b + 3][1])
    assert re.fullmatch(STAMP, code[b + 4][1]) and code[b + 5][1].startswith("je ")
    push = at(code, target(code[b + 5][1]))
    assert code[push][1] == "mov $0x18,%edi" and "operator new(unsigned long)" in code[push + 1][1]
    hook = [i for i in calls(code, "_List_node_base::_M_hook") if i > childs[0]]
    assert len(hook) == 1 and push < hook[0] < nxt and nxt - hook[0] <= 3
    # unequal falls into the pose block, which runs into the push_back: no jump over it
    assert "KeyFrame::GetPose()" in code[b + 9][1]
    block = code[b + 6:push]
    # GetPose() * Twc, * mTcwGBA, mTcwGBA.R.t() * GetRotation(), Rcor * GetVelocity(): the caller's arithmetic
    assert len([1 for _, t in block if t.startswith("call") and "cv::operator*" in t]) == 4
    assert not [t for _, t in block if t.startswith("jmp ") and skip <= target(t) <= code[nxt][0]]
    assert "cv::fastFree" in code[push - 1][1]   # the block's last instruction is a call that returns into it


@BOTH
def test_front_entry_is_tested_for_nothing(fn):
    code = ins(O_LOOP, fn)
    childs = calls(code, "KeyFrame::GetChilds()")[0]
    inv = [i for i in calls(code, "KeyFrame::GetPoseInverse()") if i > childs][0]
    assert re.fullmatch(r"mov 0x10\(%rax\),%rbx", code[childs - 4][1])      # lpKFtoCheck.front()
    between = [t for _, t in code[childs - 3:inv] if not t.startswith(("mov ", "lea "))]
    assert [t.split(" [")[0] for t in between] == ["call"]                  # GetChilds alone
    # behind the child loop: mTcwBefGBA = GetPose(); SetPose(mTcwGBA), unconditionally
    inc = [i for i in calls(code, "_Rb_tree_increment") if i > childs][0]
    assert code[inc + 3][1].startswith("jne ") and "KeyFrame::GetPose()" in code[inc + 6][1]
    tail = [t for _, t in code[inc + 4:inc + 16]]
    assert any("KeyFrame::SetPose(" in t for t in tail) and not [t for t in tail if t.startswith("j")]


@BOTH
@pytest.mark.parametrize("kind, member", [("MapPoint", "0xe0"), ("MapLine", "0xd0")])
def test_feature_loop_order_of_the_tests(fn, kind, member):
    code = ins(O_LOOP, fn)
    bad, ref = calls(code, kind + "::isBad()"), calls(code, kind + "::GetReferenceKeyFrame()")
    assert len(bad) == 1 and len(ref) == 1
    b, r = bad[0], ref[0]
    assert code[b + 1][1] == "test %al,%al" and code[b + 2][1].startswith("jne ")
    assert re.fullmatch(r"cmp %rax," + member + r"\(%r\w+\)", code[b + 4][1])
    jump = code[b + 5][1]
    set_pos = calls(code, kind + "::SetWorldPos(")
    if jump.startswith("jne "):    # unequal leaves for GetReferenceKeyFrame, equal falls into SetWorldPos(mPosGBA)
        assert at(code, target(jump)) == r - 1 and any(b < i < b + 25 for i in set_pos)
    else:                          # equal leaves for SetWorldPos(mPosGBA), unequal falls into GetReferenceKeyFrame
        assert jump.startswith("je ") and r == b + 7
        dest = at(code, target(jump))
        assert any(dest < i < dest + 25 for i in calls(code, kind + "::SetWorldPos("))
    # the reference keyframe: its stamp, then mTcwBefGBA.empty(); no isBad()
    cmp_ = [i for i in range(r + 1, r + 6) if re.fullmatch(STAMP, code[i][1])]
    assert len(cmp_) == 1 and code[cmp_[0] + 1][1].startswith("jne ")
    away = target(code[cmp_[0] + 1][1])
    assert re.fullmatch(r"lea 0x100\(%r\w+\),%r13", code[cmp_[0] + 2][1])
    e = cmp_[0] + 4
    assert "cv::Mat::empty() const" in code[e][1] and code[e + 1][1] == "test %al,%al"
    assert code[e + 2][1].startswith("jne ") and target(code[e + 2][1]) == away
    assert len(calls(code, "KeyFrame::isBad()")) == 1 and calls(code, "KeyFrame::isBad()")[0] < min(b, r)


@BOTH
def test_product_sites_are_the_pair_of_isinfrustum(fn):
    frame = ins(MAIN / "src/Frame.cc.o", "ORB_SLAM3::Frame::isInFrustum(")
    ops = [t[t.find("[") + 1:-1] for _, t in frame if t.startswith("call") and "cv::operator" in t]
    assert ops[:2] == [MUL, ADD]                    # Rcw * P + tcw
    code = ins(O_LOOP, fn)
    for kind, pairs in (("MapPoint", 2), ("MapLine", 4)):
        r = calls(code, kind + "::GetReferenceKeyFrame()")[0]
        end = [i for i in calls(code, kind + "::SetWorldPos(") if i > r][0]
        seq = [(i, t[t.find("[") + 1:-1]) for i, (_, t) in enumerate(code[r:end], r)
               if t.startswith("call") and ("cv::operator" in t or "GetPoseInverse" in t or "toVector3d" in t)]
        names = [n for _, n in seq]
        inverse = "ORB_SLAM3::KeyFrame::GetPoseInverse()"
        if kind == "MapPoint":
            assert names == [MUL, ADD, inverse, MUL, ADD]
        else:
            to3d = "ORB_SLAM3::Converter::toVector3d(cv::Mat const&)"
            assert names == [MUL, ADD, MUL, ADD, inverse, MUL, ADD, to3d, MUL, ADD, to3d]
        assert names.count(MUL) == pairs and names.count(ADD) == pairs
        for (i, a), (j, b) in zip(seq, seq[1:]):
            if a == MUL:
                assert b == ADD and j - i <= 8      # the sum takes the product's MatExpr: nothing between


@BOTH
def test_no_fused_multiply_add_of_the_functions_own(fn):
    code = ins(O_LOOP, fn)
    assert len(code) > 1000 and not [t for _, t in code if FMA.match(t)]
