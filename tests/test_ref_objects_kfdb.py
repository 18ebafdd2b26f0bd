"""Static pins, from the reference's own compiled objects, of what plvi_kfdb_query (csrc/kfdb.hip) and
tests/native/kfdb_ref.cpp restate of L1Scoring::score (ScoringObject.cpp:23-68) and of
KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates (KeyFrameDatabase.cc:790-902 / :619-787)
-- same method and helpers as tests/test_ref_objects.py: the objects are only read with objdump, never run or
loaded; the module skips where the reference build tree is absent.

* L1Scoring::score: vi is the FIRST argument's value (0x28 off v1's node), wi the second's; the term is
  subsd(vi, wi), andpd with the abs mask, subsd |vi|, subsd |wi|, then one addsd into the running sum -- three
  roundings and an add, nothing fused in the whole object; the result is xorpd with the sign mask and mulsd by 0.5;
* minCommonWords: vcvtsi2ss of maxCommonWords, vmulss by the float 0.8f, vcvttss2si (truncation);
* si: the double returned by the virtual score call is rounded once, vcvtsd2ss, and that float is both stored into
  the keyframe's score member and pushed into lScoreAndMatch;
* accumulation: the neighbour's stamp is compared with the query id (jne skips), the MEMBER is loaded and added
  with vaddss; pBestKF moves on `vcomiss bestScore, member` + cmova (strictly above, false on NaN) and bestScore is
  the vmaxss of the two;
* mode 0: vmulss by 0.75f, and `vcomiss minScoreToRetain, si` + jbe drops an entry at or below it;
* mode 1: std::list<pair<float, KeyFrame*>>::sort instantiated on a function pointer, called with compFirst."""
import re

from test_ref_objects import MAIN, REF, _disasm, _find, _fn, _rodata, pytestmark  # noqa: F401

O_SC = REF / "Thirdparty/DBoW2/build/CMakeFiles/DBoW2.dir/DBoW2/ScoringObject.cpp.o"
O_DB = MAIN / "src/KeyFrameDatabase.cc.o"
RELOC = "ORB_SLAM3::KeyFrameDatabase::DetectRelocalizationCandidates("
NBEST = "ORB_SLAM3::KeyFrameDatabase::DetectNBestCandidates("
ANY_FUSED = re.compile(r"^v?f(n)?m(add|sub)")


def test_l1_score_is_three_subtractions_and_an_add_in_that_order():
    f = _fn(O_SC, "DBoW2::L1Scoring::score(")
    # rbp walks v1 (the query), r12 walks v2: xmm2 = vi, xmm1 = wi
    assert _find(f, ["movsd 0x28(%rbp),%xmm2", "movsd 0x28(%r12),%xmm1", "movapd %xmm2,%xmm0",
                     "andpd 0x0(%rip),%xmm2 [.LC4]", "subsd %xmm1,%xmm0", "andpd 0x0(%rip),%xmm0 [.LC4]",
                     "andpd 0x0(%rip),%xmm1 [.LC4]", "subsd %xmm2,%xmm0", "subsd %xmm1,%xmm0", "addsd %xmm0,%xmm3"],
                 gap=2) == 1
    assert sum(s.startswith("subsd ") for s in f) == 3 and sum(s.startswith("addsd ") for s in f) == 1
    assert _rodata(O_SC, ".LC4", "Q") == 0x7fffffffffffffff          # fabs
    assert f.count("pxor %xmm3,%xmm3") == 1                          # score = 0


def test_l1_score_is_negated_and_halved():
    f = _fn(O_SC, "DBoW2::L1Scoring::score(")
    assert _find(f, ["xorpd 0x0(%rip),%xmm3 [.LC2]", "movsd 0x0(%rip),%xmm0 [.LC3]", "mulsd %xmm3,%xmm0", "ret"],
                 gap=8) == 1
    assert _rodata(O_SC, ".LC2", "Q") == 0x8000000000000000 and _rodata(O_SC, ".LC3", "d") == 0.5
    assert not any(s.startswith("divsd") for s in f)


def test_scoring_object_holds_no_fused_instruction():
    for name, ins in _disasm(O_SC).items():
        assert not any(ANY_FUSED.match(s) for s in ins), name


def test_min_common_words_is_a_truncated_float_product():
    for name in (RELOC, NBEST):
        f = _fn(O_DB, name)
        assert _find(f, ["vcvtsi2ss %edx,%xmm0,%xmm0", "vmulss 0x0(%rip),%xmm0,%xmm0 [.LC12]"], gap=4) == 1
        assert sum(s.startswith("vcvttss2si %xmm0,") for s in f) == 1
        i = f.index("vmulss 0x0(%rip),%xmm0,%xmm0 [.LC12]")
        assert any(s.startswith("vcvttss2si %xmm0,") for s in f[i + 1:i + 4])
        assert not any(s.startswith(("vcvtss2si ", "vroundss")) for s in f)
    assert _rodata(O_DB, ".LC12", "f") == 0.800000011920929          # 0.8f, not the double 0.8


def test_score_is_rounded_to_float_once_and_stored_into_the_member():
    for name, member in ((RELOC, "0x74(%rbp)"), (NBEST, "0x94(%rbp)")):
        f = _fn(O_DB, name)
        assert f.count("vcvtsd2ss %xmm0,%xmm0,%xmm5") == 1 and sum(s.startswith("vcvtsd2ss") for s in f) == 1
        i = f.index("vcvtsd2ss %xmm0,%xmm0,%xmm5")
        assert f[i - 1] == "call *(%rax)"                            # mpVoc->score through the scoring object
        assert f"vmovss %xmm5,{member}" in f[i + 1:i + 5]
        assert any(s == "vmovss %xmm5,0x10(%rax)" for s in f[i + 1:i + 12])  # the pair's first, in the new list node


def test_accumulation_adds_the_member_and_moves_best_on_strictly_above():
    for name, stamp, member, acc in ((RELOC, "0x68(%rdx)", "0x74(%rdx)", "(%rsp)"),
                                     (NBEST, "0x88(%rdx)", "0x94(%rdx)", "0x8(%rsp)")):
        f = _fn(O_DB, name)
        assert _find(f, [f"cmp %rsi,{stamp}", "jne", f"vmovss {member},%xmm0", f"vaddss {acc},%xmm0,%xmm2",
                         "vcomiss %xmm1,%xmm0", "vmaxss %xmm1,%xmm0,%xmm1", f"vmovss %xmm2,{acc}",
                         "cmova %rdx,%rbx"], gap=2) == 1
        assert sum(s.startswith("vaddss") for s in f) == 1
        assert not any(ANY_FUSED.match(s) for s in f)


def test_mode0_keeps_entries_strictly_above_three_quarters_of_the_best():
    f = _fn(O_DB, RELOC)
    # bestAccScore = max(accScore, bestAccScore), then * 0.75f
    assert sum(s.startswith("vmaxss 0x8(%rsp),%xmm4,") for s in f) == 1
    assert f.count("vmulss 0x0(%rip),%xmm7,%xmm7 [.LC13]") == 1 and _rodata(O_DB, ".LC13", "f") == 0.75
    assert _find(f, ["vmovss 0x10(%rbx),%xmm0", "vcomiss (%rsp),%xmm0", "jbe", "call [ORB_SLAM3::KeyFrame::GetMap]"],
                 gap=4) == 1
    # the map test comes before the insertion into spAlreadyAddedKF
    i = f.index("vcomiss (%rsp),%xmm0")
    rest = f[i:]
    ins = next(k for k, s in enumerate(rest) if "_M_insert_unique" in s)
    assert any(s == "call [ORB_SLAM3::KeyFrame::GetMap]" for s in rest[:ins])


def test_mode1_sorts_the_list_with_a_function_pointer_comparator():
    f = _fn(O_DB, NBEST)
    sort = [s for s in f if s.startswith("call [void std::__cxx11::list<std::pair<float, ORB_SLAM3::KeyFrame*>,")]
    assert len(sort) == 1 and sort[0].endswith("::sort<bool ]")     # sort<bool (*)(pair const&, pair const&)>
    i = f.index(sort[0])
    assert "mov 0x0(%rip),%rsi [ORB_SLAM3::compFirst]" in f[i - 3:i]
    assert not any("sort" in s for s in _fn(O_DB, RELOC))            # mode 0's output is not sorted
    # compFirst itself: a.first > b.first
    c = _fn(O_DB, "ORB_SLAM3::compFirst(")
    assert sum(s.startswith(("vcomiss", "comiss")) for s in c) == 1 and any(s.startswith("seta") for s in c)
