"""Static pins on the reference's KeyFrame.cc.o for the covisibility graph (csrc/covis.hip,
tests/native/covis_ref.cpp), read with objdump only:

* UpdateConnections and UpdateConnectionsWithLines compare a counter entry's count (0x28 off the map node) with
  nmax and skip the update with `jle` -- strictly above, so the FIRST keyframe of the largest count is pKFmax -- and
  take the AddConnection path behind `cmp $0xe` / `jg`: a count >= 15;
* AddConnection's equal-value path (the node's value compared with the weight, `je`) cannot reach the call of
  UpdateBestCovisibles;
* EraseConnection reaches UpdateBestCovisibles only through the erase of the map entry;
* UpdateBestCovisibles calls isBad once per pair and both push_front's lie behind its `jne`.

The three reachability pins walk the function's own branch graph (conditional branches both ways, calls of the
noreturn helpers end a path).  The module skips where the reference's build tree is absent."""
import re
import subprocess

import pytest

from test_ref_objects import MAIN, _fn, pytestmark  # noqa: F401

O_KF = MAIN / "src/KeyFrame.cc.o"
UBC = "call [ORB_SLAM3::KeyFrame::UpdateBestCovisibles]"
NORETURN = ("__throw", "__stack_chk_fail", "_Unwind_Resume")

_flows = {}


def _flow(prefix):
    """The instructions of one function as (address, text, branch target or None); text as test_ref_objects has it."""
    if prefix in _flows:
        return _flows[prefix]
    out = subprocess.run(["objdump", "-dr", "--no-show-raw-insn", "-C", str(O_KF)], capture_output=True, text=True,
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


def _reach(flow, start, without=(), cut_fallthrough=()):
    """Indices reachable from index `start`; `without`: indices that end a path; `cut_fallthrough`: conditional
    branches taken only."""
    at = {a: i for i, (a, _, _) in enumerate(flow)}
    seen, todo = set(), [start]
    while todo:
        i = todo.pop()
        if i in seen or i in without or i >= len(flow):
            continue
        seen.add(i)
        _, ins, tg = flow[i]
        op = ins.split(" ")[0]
        if op in ("ret", "retq") or (op == "call" and any(n in ins for n in NORETURN)):
            continue
        if op.startswith("j") and tg in at:
            todo.append(at[tg])
        if op == "jmp" or i in cut_fallthrough:
            continue
        todo.append(i + 1)
    return seen


def _idx(flow, text):
    return [i for i, (_, ins, _) in enumerate(flow) if ins == text]


@pytest.mark.parametrize("fn", ["UpdateConnections(", "UpdateConnectionsWithLines("])
def test_walk_is_strictly_above_and_at_least_15(fn):
    flow = _flow("ORB_SLAM3::KeyFrame::" + fn)
    ins = [t for _, t, _ in flow]
    at = {a: i for i, (a, _, _) in enumerate(flow)}
    hits = [i for i in range(len(ins) - 6) if ins[i] == "mov 0x28(%rbp),%eax" and
            re.fullmatch(r"cmp 0x[0-9a-f]+\(%rsp\),%eax", ins[i + 1]) and ins[i + 2] == "jle"]
    assert len(hits) == 1
    i = hits[0]
    nmax = ins[i + 1].split(" ")[1].split(",")[0]
    assert ins[i + 3] == f"mov %eax,{nmax}"                      # nmax = mit->second, behind the jle
    assert at[flow[i + 2][2]] > i + 3                            # ... which the jle skips: `>` and not `>=`
    j = ins.index("cmp $0xe,%eax", i)
    assert j <= i + 6 and ins[j + 1] == "jg"                     # second >= 15
    add = _idx(flow, "call [ORB_SLAM3::KeyFrame::AddConnection]")
    assert len(add) == 2                                         # the loop's (:559) and pKFmax's (:566)
    assert add[0] in _reach(flow, at[flow[j + 1][2]], without={j + 2})
    assert ins[add[0] - 2] == "lea 0x28(%rbp),%rdx"              # the weight handed over is the node's count


def test_add_connection_equal_value_returns_without_resort():
    flow = _flow("ORB_SLAM3::KeyFrame::AddConnection(")
    ins = [t for _, t, _ in flow]
    at = {a: i for i, (a, _, _) in enumerate(flow)}
    call = _idx(flow, UBC)
    assert len(call) == 1 and call[0] in _reach(flow, 0)
    eq = [i for i in range(len(ins) - 1) if re.fullmatch(r"cmp (0x28\(%r\w+\),%eax|%eax,0x28\(%r\w+\))", ins[i]) and
          ins[i + 1] == "je"]
    assert eq                                                    # mConnectedKeyFrameWeights[pKF] != weight
    for i in eq:
        assert call[0] not in _reach(flow, at[flow[i + 1][2]])   # equal: the `else return` of :209
        assert call[0] in _reach(flow, i + 2)                    # different: stored, then re-sorted
    assert any(re.fullmatch(r"mov %e\w+,0x28\(%r\w+\)", t) for t in ins)


def test_erase_connection_resorts_only_behind_the_erase():
    flow = _flow("ORB_SLAM3::KeyFrame::EraseConnection(")
    call = _idx(flow, UBC)
    erase = [i for i, (_, t, _) in enumerate(flow) if t.startswith("call [std::_Rb_tree<ORB_SLAM3::KeyFrame*") and
             t.endswith("::erase]")]
    assert len(call) == 1 and len(erase) == 1
    assert call[0] in _reach(flow, 0)
    assert call[0] not in _reach(flow, 0, without=set(erase))    # bUpdate: no path round the erase


def test_update_best_covisibles_tests_is_bad_before_both_pushes():
    flow = _flow("ORB_SLAM3::KeyFrame::UpdateBestCovisibles(")
    ins = [t for _, t, _ in flow]
    bad = _idx(flow, "call [ORB_SLAM3::KeyFrame::isBad]")
    hook = _idx(flow, "call [std::__detail::_List_node_base::_M_hook]")
    assert len(bad) == 1 and len(hook) == 2
    b = bad[0]
    assert ins[b + 1] == "test %al,%al" and ins[b + 2] == "jne"
    assert b < hook[0] < hook[1] < b + 30
    assert all(h in _reach(flow, 0) for h in hook)
    # with the jne always taken (every pair bad) neither push_front is reached
    assert not any(h in _reach(flow, 0, cut_fallthrough={b + 2}) for h in hook)
    assert _fn(O_KF, "ORB_SLAM3::KeyFrame::UpdateBestCovisibles(").count("call [ORB_SLAM3::KeyFrame::isBad]") == 1
