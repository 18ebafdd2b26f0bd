"""Static pins, from the reference's own compiled objects, of the arithmetic
csrc/triangulation.hip and tests/native/triangulation_ref.cpp restate (same
method and helpers as tests/test_ref_objects.py: the objects are only read
with objdump, never run or loaded; the module skips where the reference
build tree is absent).

* Pinhole::epipolarConstrain (Pinhole.cpp:143-156, Pinhole.cpp.o): which
  products of a, b, c, num and den the build fused, and the double compare
  of dsqr with 3.84 * unc;
* ORBmatcher::SearchForTriangulation (ORBmatcher.cc:965-1206,
  ORBmatcher.cc.o): the epipole test's one fused product, the compare GCC
  made of `dist>TH_LOW || dist>bestDist`, where bestDist is written, and
  that vbMatched2 is read but never written.
"""
import collections
import re

from test_ref_objects import O_OM, O_PIN, _find, _fn, _fused, _rodata, pytestmark  # noqa: F401

EPI = "ORB_SLAM3::Pinhole::epipolarConstrain("
SFT = ("ORB_SLAM3::ORBmatcher::SearchForTriangulation(ORB_SLAM3::KeyFrame*, ORB_SLAM3::KeyFrame*, cv::Mat, "
       "std::vector<std::pair<unsigned long, unsigned long>, std::allocator<std::pair<unsigned long, unsigned long> > "
       ">&, bool, bool)")


def test_epipolar_constrain_fused_sites_and_double_compare():
    """rax = F12.data, rdx = F12.step, rcx = &kp1 (x -> xmm3, y -> xmm0), then rax = &kp2 (x -> xmm6, y -> xmm5):
      b   = fma(x1, F01, y1*F11) + F21          (xmm1)
      a   = fma(x1, F00, y1*F10) + F20          (xmm2)
      den = fma(a, a, b*b)                      (xmm4), compared with 0.0f, equal -> return false
      c   = fma(y1, F12, x1*F02) + F22          (the RIGHT product is the fused one)
      num = c + fma(b, y2, a*x2)
      dsqr = num*num / den in float; return 3.84 * (double)unc > (double)dsqr (vcomisd + seta)."""
    f = _fn(O_PIN, EPI)
    assert _fused(f) == collections.Counter({"vfmadd231ss": 3, "vfmadd132ss": 2})
    assert _find(f, ["vmovss 0x8(%rax),%xmm9", "vmovss 0x4(%rcx),%xmm0", "vmovss (%rcx),%xmm3",
                     "vmulss 0x4(%rax,%rdx,1),%xmm0,%xmm1", "vmovss 0x8(%rax,%rdx,1),%xmm8",
                     "vfmadd231ss 0x4(%rax),%xmm3,%xmm1", "vmovss 0x8(%rax,%rdx,2),%xmm7",
                     "vaddss 0x4(%rax,%rdx,2),%xmm1,%xmm1", "vmulss (%rax,%rdx,1),%xmm0,%xmm2",
                     "vfmadd231ss (%rax),%xmm3,%xmm2", "vaddss (%rax,%rdx,2),%xmm2,%xmm2"], gap=1) == 1
    assert _find(f, ["vmulss %xmm1,%xmm1,%xmm4", "vmovss (%rax),%xmm6", "vmovss 0x4(%rax),%xmm5",
                     "vfmadd231ss %xmm2,%xmm2,%xmm4", "vucomiss 0x0(%rip),%xmm4 [.LC8]", "jnp",
                     "vmulss %xmm9,%xmm3,%xmm3", "vmulss %xmm2,%xmm6,%xmm2", "vfmadd132ss %xmm8,%xmm3,%xmm0",
                     "vfmadd132ss %xmm5,%xmm2,%xmm1", "vaddss %xmm7,%xmm0,%xmm0", "vaddss %xmm1,%xmm0,%xmm0"],
                 gap=1) == 1
    assert _find(f, ["vcvtss2sd 0x34(%rsp),%xmm1,%xmm1", "vmulsd 0x0(%rip),%xmm1,%xmm1 [.LC21]",
                     "vmulss %xmm0,%xmm0,%xmm0", "vdivss %xmm4,%xmm0,%xmm0", "vcvtss2sd %xmm0,%xmm0,%xmm0",
                     "vcomisd %xmm0,%xmm1", "seta %r12b"], gap=1) == 1
    assert _rodata(O_PIN, ".LC8", "f") == 0.0 and _rodata(O_PIN, ".LC21", "d") == 3.84
    # unc is the last float argument (xmm1 on entry), spilled to 0x34(%rsp); sigmaLevel (xmm0) is never used
    assert "vmovss %xmm1,0x34(%rsp)" in f


def test_search_for_triangulation_epipole_test():
    """distex = ep.x - kp2.pt.x (xmm0), distey = ep.y - kp2.pt.y (xmm1): fma(distex, distex, distey*distey),
    the function's only fused operation, against 100.0f * mvScaleFactors[kp2.octave]; `jbe` leaves the
    `continue` when 100*sf <= lhs (or unordered), i.e. the skip is the strict lhs < 100*sf."""
    f = _fn(O_OM, SFT)
    assert _fused(f) == collections.Counter({"vfmadd132ss": 1})
    assert _find(f, ["vsubss 0x4(%rax),%xmm1,%xmm1", "vsubss (%rax),%xmm0,%xmm0", "movslq 0x14(%rax),%rdx",
                     "vmulss %xmm1,%xmm1,%xmm1", "vmovss (%rcx,%rdx,4),%xmm7", "lea 0x0(,%rdx,4),%rax",
                     "vfmadd132ss %xmm0,%xmm1,%xmm0", "vmulss 0x0(%rip),%xmm7,%xmm1 [.LC39]", "vcomiss %xmm0,%xmm1",
                     "jbe"], gap=1) == 1
    assert _rodata(O_OM, ".LC39", "f") == 100.0


def test_search_for_triangulation_best_dist_rule():
    """bestDist lives at -0x10f4(%rbp): set to TH_LOW = 0x32 per KF1 keypoint, and written in one other place,
    after `epipolarConstrain(...) || bCoarse` (the virtual call, then the bCoarse byte) -- never on a
    rejected candidate.  `dist>TH_LOW || dist>bestDist` became the single signed compare bestDist < dist
    (bestDist never exceeds TH_LOW): an equal distance goes on, so the last one wins."""
    f = _fn(O_OM, SFT)
    assert _find(f, ["call [ORB_SLAM3::ORBmatcher::DescriptorDistance]", "mov %eax,-0x10f8(%rbp)",
                     "cmp %eax,-0x10f4(%rbp)", "jl"], gap=1) == 1
    assert _find(f, ["call *0x68(%r10)", "test %al,%al", "jne", "cmpb $0x0,-0x1157(%rbp)", "je",
                     "mov -0x1068(%rbp),%eax", "mov %eax,-0x10c4(%rbp)", "mov -0x10f8(%rbp),%eax",
                     "mov %eax,-0x10f4(%rbp)"], gap=1) == 1
    writes = [s for s in f if s.endswith(",-0x10f4(%rbp)") and not s.startswith("cmp")]
    assert sorted(set(writes)) == ["mov %eax,-0x10f4(%rbp)", "movl $0x32,-0x10f4(%rbp)"]
    assert writes.count("mov %eax,-0x10f4(%rbp)") == 1


def test_search_for_triangulation_never_writes_vbmatched2():
    """vbMatched2 is a std::vector<bool>: `vbMatched2[idx2]` is read as word & (1 << (idx2 & 63)) (the
    shlx / shr $6 / and below, or-ed with pMP2 for the `continue`), and an element assignment would be an
    `or` / `and` of a register into the word in memory.  The function holds no read-modify-write logic
    instruction with a memory destination at all, except the stack probe `orq $0x0,(%rsp)`.

    What the disassembly cannot show: that no plain `mov` store ever lands in the bitmap through another
    pointer.  libstdc++'s _Bit_reference::operator= compiles to the or / and forms only, and the source
    has no assignment to vbMatched2 (ORBmatcher.cc:1011 and :1067 are its only uses)."""
    f = _fn(O_OM, SFT)
    assert _find(f, ["call [ORB_SLAM3::KeyFrame::GetMapPoint]", "mov -0x1068(%rbp),%rdx", "mov -0x1040(%rbp),%rcx",
                     "mov %rax,%r8", "mov $0x1,%eax", "mov %r8,%rbx", "mov %rdx,%rsi", "shlx %rdx,%rax,%rax",
                     "shr $0x6,%rsi", "and (%rcx,%rsi,8),%rax", "or %rax,%rbx", "jne"], gap=1) == 1
    # (AT&T syntax: the destination is the last operand)
    rmw = re.compile(r"^(lock )?(or|and|xor|bts|btr|btc|not|neg)[bwlq]? (.*,)?(-?0x[0-9a-f]+)?\([^()]*\)$")
    assert [s for s in f if rmw.match(s)] == ["orq $0x0,(%rsp)"]
    # the bitmap's word pointer (-0x1040(%rbp)) is loaded for that read and for the vector's release only
    assert sum(1 for s in f if s.startswith("mov -0x1040(%rbp),")) <= 3


def test_keyframe_fields_read_by_the_candidate_loop():
    """kp2.octave (KeyPoint + 0x14) indexes pKF2's mvScaleFactors for the epipole test and pKF2's
    mvLevelSigma2 for `unc` (xmm1 of the virtual call); kp1.octave only feeds the unused sigmaLevel."""
    f = _fn(O_OM, SFT)
    assert _find(f, ["mov 0x780(%r15),%rdx", "movslq 0x14(%r11),%rsi", "mov 0x780(%rcx),%rcx", "mov (%rdi),%r10",
                     "vmovss (%rdx,%rax,1),%xmm1", "mov %r11,%rdx", "vmovss (%rcx,%rsi,4),%xmm0"], gap=1) == 1

