"""Static pins, from the reference's own compiled objects, of what plvi_distinctive_descriptors
(csrc/distinctive.hip) and tests/native/distinctive_ref.cpp restate of MapPoint::ComputeDistinctiveDescriptors
(MapPoint.cc:330-404) and MapLine::ComputeDistinctiveDescriptors (MapLine.cc:264-331) -- same method and helpers
as tests/test_ref_objects.py: the objects are only read with objdump, never run or loaded; the module skips where
the reference build tree is absent.

* both bodies call ORBmatcher::DescriptorDistance(cv::Mat const&, cv::Mat const&), the plain 256-bit popcount, and
  hold no relocation to LineMatcher::DescriptorDistance (whose >> 25 quirk halves every word's count): the
  MapLine's distances are the MapPoint's;
* the row of float Distances is copied into the vector<int> with truncating conversions (eight at a time with
  vcvttps2dq, the tail with vcvttss2si) -- exact, every value is an integer <= 256 -- and sorted by std::sort
  (__introsort_loop on int iterators with operator<);
* the median index is (size_t)(0.5 * (double)(N - 1)): an unsigned-to-double conversion, vmulsd with 0.5 and a
  truncating vcvttsd2si, i.e. floor((N-1)/2), the lower middle for an even N;
* BestMedian starts at INT_MAX and is replaced on a signed strict compare (median < BestMedian): the first row
  with the smallest median wins."""
from test_ref_objects import MAIN, _find, _fn, _rodata, pytestmark  # noqa: F401

O_MP = MAIN / "src/MapPoint.cc.o"
O_ML = MAIN / "src/MapLine.cc.o"
DD = "call [ORB_SLAM3::ORBmatcher::DescriptorDistance]"
SORT = ("call [void std::__introsort_loop<__gnu_cxx::__normal_iterator<int*, std::vector<int, std::allocator<int> > >, "
        "long, __gnu_cxx::__ops::_Iter_less_iter>]")
BODIES = ((O_MP, "ORB_SLAM3::MapPoint::ComputeDistinctiveDescriptors(", ".LC32"),
          (O_ML, "ORB_SLAM3::MapLine::ComputeDistinctiveDescriptors(", ".LC17"))


def test_both_bodies_call_the_orbmatcher_distance():
    for obj, name, _ in BODIES:
        f = _fn(obj, name)
        assert f.count(DD) == 1
        assert not any("LineMatcher" in s for s in f)
        # the distance comes back in eax and is stored as a float at [i][j] and [j][i]
        i = f.index(DD)
        win = f[i:i + 14]
        assert any(s.startswith("vcvtsi2ss %eax,") for s in win), win
        assert sum(s.startswith("vmovss %xmm") for s in win) >= 2, win


def test_distance_row_is_truncated_to_int_and_sorted():
    for obj, name, _ in BODIES:
        f = _fn(obj, name)
        assert sum(s == "vcvttps2dq %ymm0,%ymm0" for s in f) == 1
        assert sum(s.startswith("vcvttss2si ") for s in f) == 7  # the scalar tail of the eight-wide copy
        assert not any(s.startswith(("vcvtss2si ", "vcvtps2dq ", "vroundss", "vroundps")) for s in f)
        assert f.count(SORT) == 1
        assert f.index("vcvttps2dq %ymm0,%ymm0") < f.index(SORT)


def test_median_index_is_a_truncated_half():
    """rax = N - 1 (`js`: the conversion of a size_t with the top bit set takes the halving path); xmm0 =
    (double)rax * 0.5; rax = trunc(xmm0) (below 2^63: `jae` takes the unsigned fix-up); median = vDists[rax]."""
    for obj, name, half in BODIES:
        f = _fn(obj, name)
        assert _find(f, ["sub $0x1,%rax", "js", "vcvtsi2sd %rax,%xmm4,%xmm0", f"vmulsd 0x0(%rip),%xmm0,%xmm0 [{half}]",
                         "jae", "vcvttsd2si %xmm0,%rax", "mov (%r14,%rax,4),%eax"], gap=3) == 1
        assert _rodata(obj, half, "d") == 0.5
        assert not any(s.startswith("vcvtsd2si ") for s in f)  # every double-to-int conversion truncates


def test_best_median_update_is_signed_and_strict():
    """BestMedian = INT_MAX; MapPoint.cc.o: `cmp BestMedian,%eax / jge` skips the update when median >= BestMedian;
    MapLine.cc.o holds the operands the other way round: `cmp %eax,BestMedian / jle`.  Both are signed and keep the
    earlier row on a tie."""
    f = _fn(O_MP, BODIES[0][1])
    assert f.count("movl $0x7fffffff,-0x148(%rbp)") == 1
    assert _find(f, ["mov (%r14,%rax,4),%eax", "cmp -0x148(%rbp),%eax", "jge", "mov %eax,-0x148(%rbp)"], gap=2) >= 1
    assert not any(s in ("jae", "jbe", "ja", "jb") for s in
                   [f[i + 1] for i, s in enumerate(f[:-1]) if s == "cmp -0x148(%rbp),%eax"])
    g = _fn(O_ML, BODIES[1][1])
    assert g.count("movl $0x7fffffff,-0x150(%rbp)") == 1
    assert _find(g, ["mov (%r14,%rax,4),%eax", "cmp %eax,-0x150(%rbp)", "jle", "mov %eax,-0x150(%rbp)"], gap=2) >= 1
