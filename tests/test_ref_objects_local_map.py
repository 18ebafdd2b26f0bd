"""Static pins, from the reference's own compiled object, of what plvi_local_map (csrc/local_map.hip) and
tests/native/local_map_ref.cpp restate of Tracking::UpdateLocalKeyFrames / UpdateLocalKeyFramesWithLines
(Tracking.cc:5399-5551 / :5553-5745) -- same method and helpers as tests/test_ref_objects.py: the object is only read
with objdump, never run or loaded; the module skips where the reference build tree is absent.

* reserve: the argument is keyframeCounter.size() + 2 * size(), one lea (%rax,%rax,2) -- the 3 * of :5453;
* the vote maximum: it->second (0x28 off the map node) is compared with max as SIGNED ints and `jle` skips: strictly
  above;
* size() > 80: the vector's byte length is compared UNSIGNED with 0x287 = 8 * 81 - 1 (`ja` leaves before the first
  visit, `jbe` is the loop's back edge);
* the temporal step: byte length above 0x27f = 8 * 80 - 1 skips it (size() < 80), and the round counter starts at 20;
* the parent branch: after the push_back and the stamp the code destroys the two per-visit copies and jumps to the
  SAME address as the size() > 80 exit -- the first instruction after the outer loop (the mSensor test of :5527) --
  not to the loop's increment."""
import re
import subprocess

import pytest

from test_ref_objects import MAIN, _find, _fn, pytestmark  # noqa: F401

O_TR = MAIN / "src/Tracking.cc.o"
FUNCS = ("ORB_SLAM3::Tracking::UpdateLocalKeyFrames(", "ORB_SLAM3::Tracking::UpdateLocalKeyFramesWithLines(")

_raw_cache = {}


def _raw(prefix):
    """[(address, instruction, branch target or None, relocation symbol or None)] of one function, addresses kept."""
    if not _raw_cache:
        txt = subprocess.run(["objdump", "-d", "-r", "-C", "--no-show-raw-insn", str(O_TR)], capture_output=True,
                             text=True, check=True).stdout
        name, cur = None, None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                name, cur = m.group(1), []
                _raw_cache[name] = cur
                continue
            if cur is None:
                continue
            m = re.match(r"^\s*([0-9a-f]+):\s+(\S.*)$", line)
            if not m:
                continue
            if m.group(2).startswith("R_X86_64"):
                if cur:
                    cur[-1][3] = m.group(2).split(None, 1)[1]
                continue
            ins = re.sub(r"\s+", " ", m.group(2)).strip()
            t = re.match(r"^(j\w+|call) ([0-9a-f]+) <", ins)
            cur.append([int(m.group(1), 16), ins.split(" <")[0] if t else ins, int(t.group(2), 16) if t else None,
                        None])
    keys = [k for k in _raw_cache if k.startswith(prefix) and "[clone" not in k]
    assert len(keys) == 1, (prefix, keys)
    return _raw_cache[keys[0]]


@pytest.mark.parametrize("name", FUNCS)
def test_reserve_is_three_times_the_counter_size(name):
    f = _fn(O_TR, name)
    i = f.index("call [std::vector<ORB_SLAM3::KeyFrame*, std::allocator<ORB_SLAM3::KeyFrame*> >::reserve]")
    assert f[i - 1] == "lea (%rax,%rax,2),%rsi"


@pytest.mark.parametrize("name", FUNCS)
def test_vote_maximum_moves_on_signed_strictly_above(name):
    f = _fn(O_TR, name)
    # eax = it->second, a callee-saved 32-bit register = max; pKFmax and max are written on the fall-through only
    hits = []
    for i, s in enumerate(f[:-4]):
        m = re.match(r"^mov 0x28\(%(rbp|r1[0-5])\),%eax$", s)
        c = re.match(r"^cmp %(r1[0-5]d|ebp),%eax$", f[i + 1])
        if m and c and f[i + 2] == "jle" and f"mov %eax,%{c.group(1)}" in f[i + 3:i + 6]:
            hits.append(c.group(1))
    assert len(hits) == 1
    assert f.count(f"xor %{hits[0]},%{hits[0]}") >= 1   # max = 0


@pytest.mark.parametrize("name", FUNCS)
def test_expansion_limit_is_unsigned_size_above_80(name):
    f = _fn(O_TR, name)
    idx = [i for i, s in enumerate(f) if s == "cmp $0x287,%rax"]
    assert len(idx) == 2 and 0x287 == 8 * 81 - 1
    assert f[idx[0] + 1] == "ja" and f[idx[1] + 1] == "jbe"          # unsigned: size() > 80 leaves, <= 80 loops
    for i in idx:
        assert any(s.startswith("sub ") and s.endswith(",%rax") for s in f[i - 3:i])  # end - begin, in bytes
    assert f.count("movl $0xa,0x80(%rsp)") == 1                       # GetBestCovisibilityKeyFrames(10)


@pytest.mark.parametrize("name", FUNCS)
def test_temporal_step_runs_below_80_for_20_rounds(name):
    f = _fn(O_TR, name)
    assert _find(f, ["cmp $0x27f,%rax", "ja", "mov $0x14,%ebp"], gap=3) == 1 and 0x27f == 8 * 80 - 1
    assert _find(f, ["sub $0x3,%eax", "cmp $0x1,%eax"], gap=1) == 2   # IMU_MONOCULAR = 3, IMU_STEREO = 4


@pytest.mark.parametrize("name", FUNCS)
def test_parent_branch_leaves_the_outer_loop(name):
    f = _raw(name)
    at = {a: i for i, (a, _, _, _) in enumerate(f)}
    calls = [i for i, x in enumerate(f) if x[3] and "KeyFrame::GetParent()" in x[3]]
    assert len(calls) == 1
    i = calls[0]
    # if(pParent) if(pParent->mnTrackReferenceForFrame != mCurrentFrame.mnId): the jne is the insertion path
    window = f[i + 1:i + 8]
    assert [x[1].split(" ")[0] for x in window if x[2] is not None][:2] == ["je", "jne"]
    assert any(x[1] == "test %rax,%rax" for x in window) and any(x[1] == "cmp %rdx,0x30(%rax)" for x in window)
    ins_path = next(x[2] for x in window if x[1].startswith("jne"))
    j = at[ins_path]
    # the push_back and the stamp, then straight on to the first unconditional jump
    k = next(n for n in range(j, j + 60) if f[n][1].startswith("jmp"))
    body = [x[1] for x in f[j:k]]
    assert "mov %rax,(%rsi)" in body[:5] and "mov %rdx,0x30(%rax)" in body[:10]
    leave = f[k][2]
    # the size() > 80 exit and the loop's own fall-through exit are that same address
    lim = [n for n, x in enumerate(f) if x[1] == "cmp $0x287,%rax"]
    assert len(lim) == 2 and f[lim[0] + 1][1].startswith("ja") and f[lim[0] + 1][2] == leave
    assert f[lim[1] + 1][1].startswith("jbe") and f[lim[1] + 2][0] == leave
    assert f[lim[1] + 1][2] < leave                                    # the back edge goes up into the loop body
    # ... which is the mSensor test of the temporal step, not the iterator increment
    assert f[at[leave]][1] == "mov 0x30(%rbx),%eax" and f[at[leave] + 1][1] == "sub $0x3,%eax"
    # the path without an insertion (pParent NULL) does reach the increment and the end-iterator compare
    skip = next(x[2] for x in window if x[1].startswith("je"))
    rest = [x[1] for x in f[at[skip]:at[skip] + 40]]
    inc = next(n for n, s in enumerate(rest) if re.match(r"add \$0x8,%r1[0-9]$", s))
    assert rest[inc + 1].startswith("cmp ") and "(%rsp)" in rest[inc + 1] and rest[inc][-4:] in rest[inc + 1]
