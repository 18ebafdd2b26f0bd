"""Static pins, from the reference's own compiled objects, of the arithmetic the loop-closing matchers
(csrc/bow.hip search_by_bow_kf_kernel, csrc/proj.hip search_sim3_proj_kernel) and
tests/native/loop_match_ref.cpp restate (same method and helpers as tests/test_ref_objects.py: the objects
are only read with objdump, never run or loaded; the module skips where the reference build tree is absent).

* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, th, ratioHamming)
  (ORBmatcher.cc:588-704): the two fused multiply-adds of u and v after the multiplication by 1/z;
* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (:473-586): no fused
  operation, the projection is the virtual mpCamera->project call;
* both: the float z < 0 compare, the distance range compares, the double viewing-angle compare with 0.5, and
  (float)bestDist <= 50.0f * ratioHamming;
* KeyFrame::IsInImage and KeyFrame::GetFeaturesInArea (KeyFrame.cc.o): the compare directions and the cell
  arithmetic grid_window implements;
* ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (:823-963): bestDist1 < TH_LOW as `> 49`, the float
  ratio compare, and the read-modify-write of vbMatched2.
"""
import collections
import re

from test_ref_objects import MAIN, O_OM, _find, _fn, _fused, _rodata, pytestmark  # noqa: F401

O_KF = MAIN / "src/KeyFrame.cc.o"
VEC = "std::vector<ORB_SLAM3::MapPoint*, std::allocator<ORB_SLAM3::MapPoint*> >"
KVEC = "std::vector<ORB_SLAM3::KeyFrame*, std::allocator<ORB_SLAM3::KeyFrame*> >"
PROJ = f"ORB_SLAM3::ORBmatcher::SearchByProjection(ORB_SLAM3::KeyFrame*, cv::Mat, {VEC} const&, {VEC}&, int, float)"
PROJ_KFS = (f"ORB_SLAM3::ORBmatcher::SearchByProjection(ORB_SLAM3::KeyFrame*, cv::Mat, {VEC} const&, {KVEC} const&, "
            f"{VEC}&, {KVEC}&, int, float)")
BOW_KF = f"ORB_SLAM3::ORBmatcher::SearchByBoW(ORB_SLAM3::KeyFrame*, ORB_SLAM3::KeyFrame*, {VEC}&)"


def test_projection_of_the_vppointskfs_overload_is_fused():
    """xmm1 = z (compared with 0.0f first: `ja` skips when 0 > z); invz = 1.0f / z (xmm0); x = p3Dc(0) * invz
    (xmm1), y = p3Dc(1) * invz (xmm0); pKF + 0x45c.. = fx, fy, cx, cy:
      u = fma(x, fx, cx), v = fma(y, fy, cy), the function's only fused operations, then IsInImage(u, v)."""
    f = _fn(O_OM, PROJ_KFS)
    assert _fused(f) == collections.Counter({"vfmadd132ss": 2})
    assert _find(f, ["vmovss (%rax),%xmm1", "vxorps %xmm0,%xmm0,%xmm0", "vcomiss %xmm1,%xmm0", "ja",
                     "vmovss 0x0(%rip),%xmm0 [.LC11]", "vdivss %xmm1,%xmm0,%xmm0", "vmulss (%rcx),%xmm0,%xmm1"],
                 gap=2) == 1
    assert _find(f, ["vmulss (%rax),%xmm0,%xmm0", "vmovss 0x464(%rdi),%xmm5", "vmovss 0x468(%rdi),%xmm6",
                     "vfmadd132ss 0x45c(%rdi),%xmm5,%xmm1", "vfmadd132ss 0x460(%rdi),%xmm6,%xmm0",
                     "vmovss %xmm1,-0x780(%rbp)", "vmovss %xmm0,-0x77c(%rbp)",
                     "call [ORB_SLAM3::KeyFrame::IsInImage]"], gap=6) == 1
    assert _rodata(O_OM, ".LC11", "f") == 1.0


def test_projection_of_the_plain_overload_is_the_camera_call():
    """No fused operation anywhere in the function; z (xmm0) against 0.0f (`ja` skips when 0 > z), then x, y,
    z are stored as a cv::Point3f and mpCamera->project is called through the vtable (Pinhole::project is
    pinned unfused in tests/test_ref_objects.py), then IsInImage."""
    f = _fn(O_OM, PROJ)
    assert _fused(f) == collections.Counter()
    assert _find(f, ["vmovss (%rdx,%rax,1),%xmm0", "vcomiss %xmm0,%xmm1", "ja"], gap=1) == 1
    assert _find(f, ["vmovss %xmm2,-0x760(%rbp)", "vmovss %xmm1,-0x75c(%rbp)", "vmovss %xmm0,-0x758(%rbp)",
                     "call *%rax", "call [ORB_SLAM3::KeyFrame::IsInImage]"], gap=7) == 1
    assert "vdivss" not in " ".join(f[480:520])


def test_distance_angle_and_threshold_compares():
    """Both overloads: dist = (float)cv::norm(PO); min > dist skips, dist > max skips (vcomiss + ja);
    0.5 * (double)dist > PO.dot(Pn) skips (cv::Mat::dot's double in xmm1, vcomisd + ja);
    radius = (float)th * mvScaleFactors[level]; and the acceptance: (float)bestDist in xmm0, 50.0f *
    ratioHamming in xmm1, `jb` skips when the product is below bestDist -- bestDist <= TH_LOW * ratioHamming
    evaluated in float."""
    for name, dist_win, thr_win in (
            (PROJ, ["vcomiss %xmm0,%xmm5", "ja", "vcomiss -0x834(%rbp),%xmm0", "ja"],
             ["vcvtsi2ssl -0x830(%rbp),%xmm7,%xmm0", "vmovss 0x0(%rip),%xmm7 [.LC29]",
              "vmulss -0x824(%rbp),%xmm7,%xmm1", "vcomiss %xmm0,%xmm1", "jb"]),
            (PROJ_KFS, ["vcomiss %xmm0,%xmm7", "ja", "vcomiss -0x84c(%rbp),%xmm0", "ja"],
             ["vcvtsi2ssl -0x848(%rbp),%xmm5,%xmm0", "vmovss 0x0(%rip),%xmm6 [.LC29]",
              "vmulss -0x834(%rbp),%xmm6,%xmm1", "vcomiss %xmm0,%xmm1", "jb"])):
        f = _fn(O_OM, name)
        assert _find(f, ["call [cv::norm]"] + ["vcvtsd2ss %xmm0,%xmm0,%xmm0"] + dist_win, gap=3) == 1
        assert _find(f, ["call [cv::Mat::dot]", "vmovapd %xmm0,%xmm1", "vmulsd 0x0(%rip),%xmm0,%xmm0 [.LC15]",
                         "vcomisd %xmm1,%xmm0", "ja"], gap=3) == 1
        assert _find(f, thr_win, gap=1) == 1
        assert _find(f, ["call [ORB_SLAM3::MapPoint::PredictScale]", "call [ORB_SLAM3::KeyFrame::GetFeaturesInArea]"],
                     gap=20) == 1
        # the radius: th converted to float, times the level's scale factor
        i = f.index("call [ORB_SLAM3::MapPoint::PredictScale]")
        win = f[i:i + 16]
        assert any(re.match(r"vcvtsi2ssl -0x[0-9a-f]+\(%rbp\),%xmm7,%xmm0", s) for s in win)
        assert "vmulss (%rax,%rdx,4),%xmm0,%xmm0" in win
    assert _rodata(O_OM, ".LC29", "f") == 50.0 and _rodata(O_OM, ".LC15", "d") == 0.5


def test_keyframe_is_in_image_directions():
    """mnMinX.. are ints (KeyFrame + 0x7e8 minX, 0x7ec minY, 0x7f0 maxX, 0x7f4 maxY) converted to float:
    x < minX fails (jb), maxX <= x fails (jbe), y < minY fails (jb), the result is maxY > y (seta)."""
    f = _fn(O_KF, "ORB_SLAM3::KeyFrame::IsInImage(")
    assert _fused(f) == collections.Counter()
    assert f[1:17] == ["vxorps %xmm1,%xmm1,%xmm1", "vmovss (%rsi),%xmm2", "vcvtsi2ssl 0x7e8(%rdi),%xmm1,%xmm0",
                       "vcomiss %xmm0,%xmm2", "jb", "vcvtsi2ssl 0x7f0(%rdi),%xmm1,%xmm0", "vcomiss %xmm2,%xmm0", "jbe",
                       "vcvtsi2ssl 0x7ec(%rdi),%xmm1,%xmm0", "vmovss (%rdx),%xmm2", "vcomiss %xmm0,%xmm2", "jb",
                       "vcvtsi2ssl 0x7f4(%rdi),%xmm1,%xmm1", "vcomiss %xmm2,%xmm1", "seta %al", "ret"]


def test_keyframe_get_features_in_area_cell_arithmetic():
    """The Frame's arithmetic (grid_window, csrc/grid_search.h), one IEEE operation per operator:
    ((x - (float)mnMinX) - r) * mfGridElementWidthInv, floor (vroundss $9), max with 0, compared with
    mnGridCols; ((x - mnMinX) + r) * inv, ceil (vroundss $10), min with cols - 1; the same for y; and the
    candidate test r > |kp.x - x| && r > |kp.y - y| (fabs as an and-mask, vcomiss + jbe / ja)."""
    f = _fn(O_KF, "ORB_SLAM3::KeyFrame::GetFeaturesInArea(")
    assert _fused(f) == collections.Counter()
    assert _find(f, ["vcvtsi2ssl 0x7e8(%r12),%xmm2,%xmm0", "vmovss (%r14),%xmm0", "vsubss %xmm1,%xmm0,%xmm0",
                     "vsubss %xmm3,%xmm0,%xmm1", "vmulss %xmm4,%xmm1,%xmm1", "vroundss $0x9,%xmm1,%xmm1,%xmm1",
                     "vcvttss2si %xmm1,%ecx", "cmovns %ecx,%eax", "cmp %eax,%edx", "jle", "vaddss %xmm3,%xmm0,%xmm0",
                     "vmulss %xmm4,%xmm0,%xmm0", "vroundss $0xa,%xmm0,%xmm0,%xmm0", "vcvttss2si %xmm0,%eax"],
                 gap=4) == 1
    assert _find(f, ["vcvtsi2ssl 0x7ec(%r12),%xmm2,%xmm2", "vsubss %xmm2,%xmm0,%xmm2", "vsubss %xmm3,%xmm2,%xmm0",
                     "vmulss %xmm1,%xmm0,%xmm0", "vroundss $0x9,%xmm0,%xmm0,%xmm0", "vcvttss2si %xmm0,%edi",
                     "cmovns %edi,%eax", "cmp %eax,%edx", "jle", "vaddss %xmm3,%xmm2,%xmm0",
                     "vmulss %xmm1,%xmm0,%xmm0", "vroundss $0xa,%xmm0,%xmm0,%xmm0", "vcvttss2si %xmm0,%eax"],
                 gap=4) == 1
    assert _find(f, ["vsubss (%r14),%xmm0,%xmm0", "vandps 0x0(%rip),%xmm0,%xmm0 [.LC64]", "vcomiss %xmm0,%xmm1", "jbe",
                     "vmovss 0x4(%rax),%xmm0", "vandps 0x0(%rip),%xmm0,%xmm0 [.LC64]", "vcomiss %xmm0,%xmm1", "ja"],
                 gap=3) >= 1
    # the grid is 64 x 48 cells of the Frame (mnGridCols at +0x20, mnGridRows at +0x24 feed the clamps above)
    assert "mov 0x20(%r12),%edx" in f and "mov 0x24(%r12),%edx" in f


def test_search_by_bow_kf_compares_and_vbmatched2_write():
    """bestDist1 (eax) against 49: `jg` leaves when bestDist1 > 49, i.e. bestDist1 < TH_LOW is strict (the
    KF-Frame function compares <=).  Then (float)bestDist2 * mfNNratio in xmm0 against (float)bestDist1 in
    xmm1: `jbe` leaves when the product <= bestDist1.  vpMatches12[idx1] is stored and vbMatched2[bestIdx2]
    set: the read-modify-write `or` of 1 << (bestIdx2 & 63) into the bitmap word bestIdx2 >> 6.  The
    function holds no fused operation."""
    f = _fn(O_OM, BOW_KF)
    assert _fused(f) == collections.Counter()
    assert _find(f, ["cmp $0x31,%eax", "jg", "vcvtsi2ssl -0x4ac(%rbp),%xmm4,%xmm0", "vmulss (%rdi),%xmm0,%xmm0",
                     "vcvtsi2ss %eax,%xmm4,%xmm1", "vcomiss %xmm1,%xmm0", "jbe"], gap=3) == 1
    assert _find(f, ["vcomiss %xmm1,%xmm0", "jbe", "shr $0x6,%rsi", "mov %rcx,(%rax,%r10,8)", "mov $0x1,%eax",
                     "shlx %rdx,%rax,%rax", "or %rax,(%rcx,%rsi,8)"], gap=8) == 1
    # (AT&T syntax: the destination is the last operand) the only read-modify-write logic instruction with a
    # memory destination in the function is that `or`
    rmw = re.compile(r"^(lock )?(or|and|xor|bts|btr|btc)[bwlq]? (.*,)?(-?0x[0-9a-f]+)?\([^()]*\)$")
    assert [s for s in f if rmw.match(s)] == ["or %rax,(%rcx,%rsi,8)"]
    # the same bitmap is read for the `vbMatched2[idx2] || !pMP2` skip
    assert any(s.startswith("shlx %r14,%rax,%rax") for s in f)
