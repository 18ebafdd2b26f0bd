"""Static pins on the reference's MapPoint.cc.o and MapLine.cc.o for the feature refresh
(csrc/feature_refresh.hip, tests/native/feature_refresh_ref.cpp), read with objdump only.

MapPoint::UpdateNormalAndDepth() and MapLine::UpdateNormalAndDepth():
* the observer loop is GetCameraCenter, operator-(Mat, Mat), cv::norm, operator/(Mat, double),
  operator+(Mat const&, MatExpr const&) in that order, with no KeyFrame::isBad() between GetCameraCenter and
  operator- (bad observers are counted);
* behind the loop: GetCameraCenter, operator-, cv::norm, then vcvtsd2ss (dist is narrowed to float at once), one
  vmulss (dist * levelScaleFactor), one vdivss (mfMaxDistance / mvScaleFactors[nLevels - 1]), vcvtsi2sdl (n goes to
  operator/(Mat, double) as a double), operator/;
* the MapLine midpoint is vaddpd / vmulpd and vaddsd / vmulsd ahead of Converter::toCvMat: an add, then a multiply,
  in double;
* neither function holds a fused multiply-add: every float instruction outside OpenCV is the plain one.

What the calls do inside OpenCV is not pinned by these objects (parity unpinned: DESIGN.md).  The module skips where
the reference's build tree is absent."""
import re

import pytest

from test_ref_objects import MAIN, pytestmark  # noqa: F401
from test_ref_objects_essential_graph import ins

FUNCS = {"point": (MAIN / "src/MapPoint.cc.o", "ORB_SLAM3::MapPoint::UpdateNormalAndDepth()"),
         "line": (MAIN / "src/MapLine.cc.o", "ORB_SLAM3::MapLine::UpdateNormalAndDepth()")}
CALLS = {"center": "ORB_SLAM3::KeyFrame::GetCameraCenter()", "sub": "cv::operator-(cv::Mat const&, cv::Mat const&)",
         "norm": "cv::norm(cv::_InputArray const&, int, cv::_InputArray const&)",
         "div": "cv::operator/(cv::Mat const&, double)", "add": "cv::operator+(cv::Mat const&, cv::MatExpr const&)",
         "right": "ORB_SLAM3::KeyFrame::GetRightCameraCenter()", "isbad": "ORB_SLAM3::KeyFrame::isBad()",
         "tocv": "ORB_SLAM3::Converter::toCvMat(Eigen::Matrix<double, 3, 1, 0, 3, 1> const&)"}
FLOAT = re.compile(r"^(vcvtsd2ss|vcvtsi2sdl|vmulss|vdivss|vaddpd|vmulpd|vaddsd|vmulsd)\b")


def trace(kind):
    """The function as a list of tokens in address order: the names of CALLS for its calls, the mnemonics of FLOAT."""
    obj, fn = FUNCS[kind]
    body = ins(obj, fn)
    assert len(body) > 500, "function not found"
    out = []
    for _, t in body:
        if t.startswith("call") and "[" in t:
            callee = t.split("[", 1)[1].rstrip("]")
            out += [k for k, name in CALLS.items() if callee.startswith(name)]
        else:
            m = FLOAT.match(t)
            if m:
                out.append(m.group(1))
    return out, body


@pytest.mark.parametrize("kind", ("point", "line"))
def test_call_sites_and_float_instructions(kind):
    tr, _ = trace(kind)
    loop = ["center", "sub", "norm", "div", "add"]
    tail = ["center", "sub", "norm", "vcvtsd2ss", "vmulss", "vdivss", "vcvtsi2sdl", "div"]
    if kind == "point":
        # the left observer, the right observer (out of scope here), then the reference keyframe
        assert tr == loop + ["right", "sub", "norm", "div", "add"] + tail
    else:
        assert tr == ["vaddpd", "vmulpd", "vaddsd", "vmulsd", "tocv"] + loop + tail


@pytest.mark.parametrize("kind", ("point", "line"))
def test_no_isbad_in_the_observer_loop(kind):
    tr, _ = trace(kind)
    first = tr.index("center")
    assert tr[first + 1] == "sub"
    assert "isbad" not in tr        # nowhere in the function, so not between GetCameraCenter and operator-


@pytest.mark.parametrize("kind", ("point", "line"))
def test_no_fused_multiply_add(kind):
    _, body = trace(kind)
    fused = [t for _, t in body if re.match(r"^vf(n?m)(add|sub)", t)]
    assert not fused, fused[:3]
