"""Static pins, from the reference's own compiled objects, of the arithmetic the Fuse searches
(csrc/fuse.hip fuse_points_kernel / fuse_lines_kernel) and tests/native/fuse_ref.cpp restate (same method and
helpers as tests/test_ref_objects.py: the objects are only read with objdump, never run or loaded; the module
skips where the reference build tree is absent).

* ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (ORBmatcher.cc:1399-1610): three fused operations --
  ur = fnma(bf, invz, uv.x); e2 = fma(ex, ex, ey*ey), shared by both branches of the reprojection gate, and
  e2 = fma(er, er, e2) in the stereo branch --, the double compares against 7.8 / 5.99, bestDist = 256 and
  `cmp $50 / jg`;
* ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1612-1734): no fused operation, bestDist = INT_MAX;
* both: the float z < 0 compare, the virtual project call, the distance range compares, the double
  viewing-angle compare with 0.5, radius = th (a float, no conversion) * mvScaleFactors[level], the octave
  window and the strict dist < bestDist;
* LineMatcher::Fuse (LineMatcher.cpp:373-485): the four fused projections fma(f*X, invz, c), the inclusive
  bounds compares in source order, GetLinesInArea called with -1 / -1, bestDist = INT_MAX, `cmp $50 / jg`;
* KeyFrame::GetLinesInArea (KeyFrame.cc:1170-1198): the double midpoint distance with its three fused
  operations, rounded to float against r*r in float; the float slope against (double)r * 0.01 in double,
  without an absolute value; the level filter behind bCheckLevels = minLevel > 0 || maxLevel > 0."""
import collections

from test_ref_objects import MAIN, O_LM, O_OM, _find, _fn, _fused, _rodata, pytestmark  # noqa: F401

O_KF = MAIN / "src/KeyFrame.cc.o"
VEC = "std::vector<ORB_SLAM3::MapPoint*, std::allocator<ORB_SLAM3::MapPoint*> >"
LVEC = "std::vector<ORB_SLAM3::MapLine*, std::allocator<ORB_SLAM3::MapLine*> >"
FUSE = f"ORB_SLAM3::ORBmatcher::Fuse(ORB_SLAM3::KeyFrame*, {VEC} const&, float, bool)"
FUSE_SIM3 = f"ORB_SLAM3::ORBmatcher::Fuse(ORB_SLAM3::KeyFrame*, cv::Mat, {VEC} const&, float, {VEC}&)"
FUSE_LINES = f"ORB_SLAM3::LineMatcher::Fuse(ORB_SLAM3::KeyFrame*, {LVEC} const&, float)"
LINES_IN_AREA = "ORB_SLAM3::KeyFrame::GetLinesInArea("


def test_fuse_reprojection_gate_is_fused():
    """0x14(%rsp) = bf (pKF + 0x474), 0x18(%rsp) = uv.x, 0x38(%rsp) = invz = 1.0f / z:
      ur = -(bf * invz) + uv.x in one vfnmadd132ss, before the candidate loop.
    In the loop xmm2 = uv.y - kp.pt.y, xmm0 = uv.x - kp.pt.x, xmm1 = mvuRight[idx] (compared with the 0.0f at
    0x70(%rsp): `jb` takes the monocular branch when mvuRight < 0, and for a NaN):
      xmm2 = ey*ey (vmulss); xmm0 = ex*ex + xmm2 (vfmadd132ss) -- ahead of the branch, so for both;
      stereo: xmm1 = ur - kpr, xmm0 = er*er + xmm0 (vfmadd231ss), times mvInvLevelSigma2[octave], widened,
      `ja` skips when > 7.8; monocular: the same product against 5.99, `jbe` keeps it."""
    f = _fn(O_OM, FUSE)
    assert _fused(f) == collections.Counter({"vfnmadd132ss": 1, "vfmadd132ss": 1, "vfmadd231ss": 1})
    assert _find(f, ["vmovss 0x474(%r14),%xmm7", "vmovss %xmm6,0x18(%rsp)", "vmovss %xmm7,0x14(%rsp)"], gap=2) == 1
    assert _find(f, ["vmovss 0x14(%rsp),%xmm6", "vmovss 0x18(%rsp),%xmm7", "vfnmadd132ss 0x38(%rsp),%xmm7,%xmm6",
                     "movl $0x100,0x30(%rsp)", "vmovss %xmm6,0x14(%rsp)"], gap=5) == 1
    assert _find(f, ["vdivss %xmm0,%xmm1,%xmm5", "vmovss %xmm5,0x38(%rsp)"], gap=1) >= 1
    assert _find(f, ["vmovss 0xcc(%rsp),%xmm2", "vsubss 0x4(%rax),%xmm2,%xmm2", "vmovss 0xc8(%rsp),%xmm0",
                     "vsubss (%rax),%xmm0,%xmm0", "vmulss %xmm2,%xmm2,%xmm2", "vmovss (%rdi,%rdx,4),%xmm1",
                     "vcomiss 0x70(%rsp),%xmm1", "vfmadd132ss %xmm0,%xmm2,%xmm0", "vmovss (%rax,%rcx,4),%xmm2", "jb",
                     "vmovss 0x14(%rsp),%xmm5", "vsubss %xmm1,%xmm5,%xmm1", "vfmadd231ss %xmm1,%xmm1,%xmm0",
                     "vmulss %xmm2,%xmm0,%xmm0", "vcvtss2sd %xmm0,%xmm0,%xmm0",
                     "vcomisd 0x0(%rip),%xmm0 [.LC16]", "ja"], gap=3) == 1
    assert _find(f, ["vmulss %xmm2,%xmm0,%xmm0", "vcvtss2sd %xmm0,%xmm0,%xmm0", "vcomisd 0x0(%rip),%xmm0 [.LC17]",
                     "jbe"], gap=1) == 1
    assert _rodata(O_OM, ".LC16", "d") == 7.8 and _rodata(O_OM, ".LC17", "d") == 5.99
    assert _rodata(O_OM, ".LC11", "f") == 1.0


def test_fuse_sim3_overload_has_no_fused_operation():
    f = _fn(O_OM, FUSE_SIM3)
    assert _fused(f) == collections.Counter()
    assert not any(s.startswith("vcomisd 0x0(%rip)") for s in f)  # no chi-square gate


def test_fuse_best_distance_and_threshold():
    """Mode 0: bestDist = 256 (0x100), bestIdx = -1; mode 1: bestDist = INT_MAX.  Both: the octave in ecx / eax
    against nPredictedLevel (`jg` skips) and nPredictedLevel - 1 (`jl` skips); dist (eax) against bestDist with
    `jge`, i.e. strict <, the first minimum wins; bestDist against 50 with `jg`, i.e. accepted when <= TH_LOW."""
    f = _fn(O_OM, FUSE)
    assert _find(f, ["movl $0xffffffff,0x10(%rsp)", "movl $0x100,0x30(%rsp)", "sub $0x1,%ecx", "mov %ecx,0x50(%rsp)"],
                 gap=3) == 1
    assert _find(f, ["movslq 0x14(%rax),%rcx", "cmp 0x28(%rsp),%ecx", "jg", "cmp 0x50(%rsp),%ecx", "jl"], gap=1) == 1
    assert _find(f, ["call [ORB_SLAM3::ORBmatcher::DescriptorDistance]", "cmp 0x30(%rsp),%eax", "jge"], gap=1) == 1
    assert _find(f, ["cmpl $0x32,0x30(%rsp)", "jg", "call [ORB_SLAM3::KeyFrame::GetMapPoint]"], gap=8) == 1
    g = _fn(O_OM, FUSE_SIM3)
    assert _find(g, ["movl $0xffffffff,-0x828(%rbp)", "movl $0x7fffffff,-0x820(%rbp)", "sub $0x1,%ecx"], gap=1) == 1
    assert _find(g, ["mov 0x14(%rax),%eax", "cmp -0x824(%rbp),%eax", "jg", "cmp -0x7f8(%rbp),%eax", "jl"], gap=1) == 1
    assert _find(g, ["call [ORB_SLAM3::ORBmatcher::DescriptorDistance]", "cmp -0x820(%rbp),%eax", "jge"], gap=1) == 1
    assert _find(g, ["cmpl $0x32,-0x820(%rbp)", "jg", "call [ORB_SLAM3::KeyFrame::GetMapPoint]"], gap=10) == 1
    assert "movl $0x100,0x30(%rsp)" not in g and not any("$0x7fffffff," in s for s in f)


def test_fuse_depth_projection_distance_angle_radius():
    """Both overloads: z against 0.0f (`ja` skips when 0 > z); x, y, z stored as a cv::Point3f and
    mpCamera->project called through the vtable (Pinhole::project is pinned unfused in
    tests/test_ref_objects.py), then IsInImage; dist = (float)cv::norm(PO), min > dist skips, dist > max skips;
    0.5 * (double)dist > PO.dot(Pn) skips (vcomisd); radius = th * mvScaleFactors[level] with th loaded as a
    float (vmovss, no vcvtsi2ss: SearchByProjection(pKF, Scw, ...) converts an int here)."""
    for name, zcmp, store, dist_win, th_load in (
            (FUSE, ["vcomiss %xmm0,%xmm3", "ja", "vmovss 0x0(%rip),%xmm1 [.LC11]"],
             ["vmovss %xmm2,0xe0(%rsp)", "vmovss %xmm1,0xe4(%rsp)", "vmovss %xmm0,0xe8(%rsp)", "call *%rax",
              "call [ORB_SLAM3::KeyFrame::IsInImage]"],
             ["vcomiss %xmm0,%xmm6", "ja", "vcomiss 0x28(%rsp),%xmm0", "ja"], "vmovss 0x2c(%rsp),%xmm6"),
            (FUSE_SIM3, ["vcomiss %xmm0,%xmm1", "ja", "mov $0x1,%eax"],
             ["vmovss %xmm2,-0x760(%rbp)", "vmovss %xmm1,-0x75c(%rbp)", "vmovss %xmm0,-0x758(%rbp)", "call *%rax",
              "call [ORB_SLAM3::KeyFrame::IsInImage]"],
             ["vcomiss %xmm0,%xmm5", "ja", "vcomiss -0x828(%rbp),%xmm0", "ja"], "vmovss -0x7d8(%rbp),%xmm6")):
        f = _fn(O_OM, name)
        assert _find(f, zcmp, gap=1) >= 1
        assert _find(f, store, gap=7) == 1
        assert _find(f, ["call [cv::norm]", "vcvtsd2ss %xmm0,%xmm0,%xmm0"] + dist_win, gap=3) == 1
        assert _find(f, ["call [cv::Mat::dot]", "vmovapd %xmm0,%xmm1", "vmulsd 0x0(%rip),%xmm0,%xmm0 [.LC15]",
                         "vcomisd %xmm1,%xmm0", "ja"], gap=3) == 1
        i = f.index("call [ORB_SLAM3::MapPoint::PredictScale]")
        win = f[i:i + 16]
        assert th_load in win and "vmulss (%rax,%rdx,4),%xmm6,%xmm0" in win
        assert not any(s.startswith("vcvtsi2ss") for s in win)
        assert "call [ORB_SLAM3::KeyFrame::GetFeaturesInArea]" in win
    assert _rodata(O_OM, ".LC15", "d") == 0.5


def test_line_fuse_projection_bounds_and_threshold():
    """Either z against 0.0f (`ja` skips when 0 > z); invz1 = 1.0f / SpcZ (xmm0); pKF + 0x45c.. = fx, fy, cx, cy:
      u1 = (fx * SPcX) * invz1 + cx, v1 = (fy * SPcY) * invz1 + cy: vmulss then vfmadd132ss, likewise u2, v2 --
    the function's four fused operations.  Bounds: (float)mnMinX > u skips, u > (float)mnMaxX skips (`ja` both:
    equality passes at either end), then v; endpoint 1 before endpoint 2."""
    f = _fn(O_LM, FUSE_LINES)
    assert _fused(f) == collections.Counter({"vfmadd132ss": 4})
    assert _find(f, ["vxorps %xmm6,%xmm6,%xmm6", "vmovss (%rsi),%xmm0", "vcomiss %xmm0,%xmm6", "ja",
                     "vcomiss (%rax),%xmm6", "ja", "vmovss 0x0(%rip),%xmm7 [.LC13]", "vdivss %xmm0,%xmm7,%xmm0"],
                 gap=3) == 1
    assert _find(f, ["vmovss 0x45c(%rsi),%xmm4", "vmovss 0x464(%rsi),%xmm8", "vmulss (%rbx),%xmm4,%xmm1",
                     "vmovss 0x460(%rsi),%xmm5", "vmovss 0x468(%rsi),%xmm7", "vfmadd132ss %xmm0,%xmm8,%xmm1",
                     "vmulss (%rbx),%xmm5,%xmm2", "vfmadd132ss %xmm2,%xmm7,%xmm0"], gap=3) == 1
    assert _find(f, ["vcvtsi2ssl 0x7e8(%rsi),%xmm6,%xmm2", "vcomiss %xmm1,%xmm2", "ja",
                     "vcvtsi2ssl 0x7f0(%rsi),%xmm6,%xmm3", "vcomiss %xmm3,%xmm1", "ja",
                     "vcvtsi2ssl 0x7ec(%rsi),%xmm6,%xmm6", "vcomiss %xmm0,%xmm6", "ja",
                     "vcvtsi2ssl 0x7f4(%rsi),%xmm1,%xmm9", "vcomiss %xmm9,%xmm0", "ja"], gap=3) == 1
    assert _find(f, ["vmulss (%rcx),%xmm4,%xmm0", "vdivss (%rax),%xmm1,%xmm10", "vfmadd132ss %xmm10,%xmm8,%xmm0",
                     "vmulss (%rdi),%xmm5,%xmm1", "vcomiss %xmm0,%xmm2", "vfmadd132ss %xmm10,%xmm7,%xmm1", "ja",
                     "vcomiss %xmm3,%xmm0", "ja", "vcomiss %xmm1,%xmm6", "ja", "vcomiss %xmm9,%xmm1", "ja"],
                 gap=3) == 1
    assert _rodata(O_LM, ".LC13", "f") == 1.0
    # distance range, viewing angle, radius (th a float) and the call with the header's default levels -1, -1
    assert _find(f, ["call [cv::norm]", "vcvtsd2ss %xmm0,%xmm0,%xmm0", "vcomiss %xmm0,%xmm7", "ja",
                     "vcomiss -0x928(%rbp),%xmm0", "ja"], gap=3) == 1
    assert _find(f, ["call [cv::Mat::dot]", "vmovapd %xmm0,%xmm1", "vmulsd 0x0(%rip),%xmm0,%xmm0 [.LC14]",
                     "vcomisd %xmm1,%xmm0", "ja"], gap=3) == 1
    assert _rodata(O_LM, ".LC14", "d") == 0.5
    assert _find(f, ["call [ORB_SLAM3::MapLine::PredictScale]", "vmovss -0x960(%rbp),%xmm7",
                     "vmulss (%rax,%rdx,4),%xmm7,%xmm0", "push $0xffffffffffffffff", "push $0xffffffffffffffff",
                     "call [ORB_SLAM3::KeyFrame::GetLinesInArea]"], gap=8) == 1
    # bestDist = INT_MAX, the octave window, strict <, <= 50
    assert _find(f, ["movl $0xffffffff,-0x8e8(%rbp)", "movl $0x7fffffff,-0x898(%rbp)", "sub $0x1,%ecx"], gap=1) == 1
    assert _find(f, ["mov 0x8(%rax),%eax", "cmp -0x8e0(%rbp),%eax", "jl", "cmp -0x8b8(%rbp),%eax", "jg"], gap=1) == 1
    assert _find(f, ["call [ORB_SLAM3::LineMatcher::DescriptorDistance]", "cmp -0x898(%rbp),%eax", "jge"], gap=1) == 1
    assert _find(f, ["cmpl $0x32,-0x898(%rbp)", "jg"], gap=1) == 1


def test_get_lines_in_area_arithmetic():
    """Per keyline (a 68-byte copy: angle at +0, octave at +8, pt at +0xc / +0x10), xmm4 = x1, xmm5 = x2,
    xmm3 = y1, xmm6 = y2, xmm1 = r:
      dx = 0.5 * (double)(x1 + x2) - (double)pt.x   (float add, widened; vfmsub231sd with .LC66 = 0.5)
      dy likewise; dy*dy (vmulsd); dx*dx + dy*dy (vfmadd132sd); rounded to float (vcvtsd2ss) and compared with
      r*r computed in float (vmulss): `ja` skips when distance > r*r;
      slope = (y1 - y2) / (x1 - x2) - angle in float (vsubss, vsubss, vdivss, vsubss), widened, against
      (double)r * 0.01 (.LC67): `ja` skips when above -- no absolute value (no and-mask in the function), and
      a NaN passes;
      the level filter only behind bCheckLevels = minLevel > 0 || maxLevel > 0 (setg / setg / or)."""
    f = _fn(O_KF, LINES_IN_AREA)
    assert _fused(f) == collections.Counter({"vfmsub231sd": 2, "vfmadd132sd": 1})
    assert _find(f, ["vaddss %xmm5,%xmm4,%xmm0", "vcvtss2sd %xmm0,%xmm0,%xmm1", "vcvtss2sd 0xc(%rdx),%xmm7,%xmm0",
                     "vfmsub231sd 0x0(%rip),%xmm1,%xmm0 [.LC66]", "vaddss %xmm6,%xmm3,%xmm1",
                     "vcvtss2sd %xmm1,%xmm1,%xmm2", "vcvtss2sd 0x10(%rdx),%xmm7,%xmm1",
                     "vfmsub231sd 0x0(%rip),%xmm2,%xmm1 [.LC66]", "vmulsd %xmm1,%xmm1,%xmm1",
                     "vfmadd132sd %xmm0,%xmm1,%xmm0", "vmovss (%r14),%xmm1", "vmulss %xmm1,%xmm1,%xmm2",
                     "vcvtsd2ss %xmm0,%xmm0,%xmm0", "vcomiss %xmm2,%xmm0", "ja"], gap=1) == 1
    assert _find(f, ["vsubss %xmm6,%xmm3,%xmm3", "vsubss %xmm5,%xmm4,%xmm4", "vcvtss2sd %xmm1,%xmm1,%xmm1",
                     "vmulsd 0x0(%rip),%xmm1,%xmm1 [.LC67]", "vdivss %xmm4,%xmm3,%xmm3", "vsubss (%rdx),%xmm3,%xmm3",
                     "vcvtss2sd %xmm3,%xmm3,%xmm3", "vcomisd %xmm1,%xmm3", "ja"], gap=1) == 1
    assert _rodata(O_KF, ".LC66", "d") == 0.5 and _rodata(O_KF, ".LC67", "d") == 0.01
    assert not any(s.startswith(("vandps", "vandpd")) for s in f)
    assert _find(f, ["test %eax,%eax", "setg %dl", "test %esi,%esi", "setg %al", "or %eax,%edx"], gap=1) == 1
    assert _find(f, ["cmpb $0x0,0x17(%rsp)", "je", "mov 0x8(%rdx),%edx", "cmp %edx,0x18(%rbp)", "jg"], gap=1) == 1
    assert "add $0x44,%rax" in f  # the 68-byte KeyLine stride
