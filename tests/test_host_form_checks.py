"""Every host-form wrapper refuses a companion array of the wrong length, or a descriptor table that is not 32
wide, with ValueError before the library is entered (the C staging would read past the end of host memory).

Sizes are minimal: 3 keypoints (or left lines) against 2 points (or right lines).  The wrappers' call functions
are replaced: the untouched arguments must reach one (so the refusals below are the checks', not a broken
fixture), a mutated argument must not."""
import numpy as np
import pytest

import plvi
from plvi import _abi

NK, NP = 3, 2


class Reached(Exception):
    pass


def kps(n):
    return np.zeros(n, plvi.KEYPOINT_DTYPE)


def kls(n):
    return np.zeros(n, plvi.KEYLINE_DTYPE)


def arr(dtype, n, w=None):
    return np.zeros(n if w is None else (n, w), dtype)


def desc(n):
    return arr(np.uint8, n, 32)


def f32(n, w=None):
    return arr(np.float32, n, w)


def u8(n):
    return arr(np.uint8, n)


def i32(n, w=None):
    return arr(np.int32, n, w)


GRID = [[[] for _ in range(2)] for _ in range(2)]
POINTS = dict(flags=u8(NP), x3dc=f32(NP, 3), dist=f32(NP, 3), dot=arr(np.float64, NP), level=i32(NP), mp_desc=desc(NP))
PYR = [np.zeros((4, 4), np.uint8)]


def _matcher():
    return plvi.ORBmatcher()


# name -> (callable factory, keyword arguments, per-record companion arrays, descriptor tables)
CASES = {
    "SearchByBoW": (lambda: _matcher().SearchByBoW,
                    dict(kf_desc=desc(NP), kf_angle=f32(NP), kf_live=u8(NP), kf_featvec={}, f_desc=desc(NK),
                         f_angle=f32(NK), f_featvec={}),
                    ["kf_angle", "kf_live", "f_angle"], ["kf_desc", "f_desc"]),
    "SearchByBoWKF": (lambda: _matcher().SearchByBoWKF,
                      dict(desc1=desc(NK), angle1=f32(NK), live1=u8(NK), featvec1={}, desc2=desc(NP), angle2=f32(NP),
                           live2=u8(NP), featvec2={}),
                      ["angle1", "live1", "angle2", "live2"], ["desc1", "desc2"]),
    "SearchForTriangulation": (lambda: _matcher().SearchForTriangulation,
                               dict(kps1=kps(NK), desc1=desc(NK), featvec1={}, has_point1=u8(NK), uright1=f32(NK),
                                    kps2=kps(NP), desc2=desc(NP), featvec2={}, has_point2=u8(NP), uright2=f32(NP),
                                    F12=np.eye(3), ep=(0, 0), sigma2=[1.0], scale_factors=[1.0]),
                               ["desc1", "has_point1", "uright1", "desc2", "has_point2", "uright2"],
                               ["desc1", "desc2"]),
    "SearchByProjection": (lambda: _matcher().SearchByProjection,
                           dict(params=plvi.ProjParams(), cur_kps=kps(NK), cur_desc=desc(NK), last_x3dc=f32(NP, 3),
                                last_octave=i32(NP), last_angle=f32(NP), mp_desc=desc(NP), last_flags=u8(NP),
                                cur_blocked=u8(NK), cur_uright=f32(NK)),
                           ["cur_desc", "cur_blocked", "cur_uright", "last_x3dc", "last_octave", "last_angle",
                            "mp_desc"], ["cur_desc", "mp_desc"]),
    "SearchByProjectionLocal": (lambda: _matcher().SearchByProjectionLocal,
                                dict(params=plvi.LocalParams(), kps=kps(NK), desc=desc(NK), mp_flags=u8(NP),
                                     mp_proj=f32(NP, 4), mp_level=i32(NP), mp_desc=desc(NP), blocked=u8(NK),
                                     uright=f32(NK)),
                                ["desc", "blocked", "uright", "mp_proj", "mp_level", "mp_desc"], ["desc", "mp_desc"]),
    "SearchByProjectionStereo": (lambda: _matcher().SearchByProjectionStereo,
                                 dict(params=plvi.ProjParams(), kps=kps(NK), desc=desc(NK), kps_r=kps(NK),
                                      desc_r=desc(NK), x3dc=f32(NP, 3), x3dr=f32(NP, 3), last_octave=i32(NP),
                                      last_angle=f32(NP), mp_desc=desc(NP), last_flags=u8(NP), blocked=u8(NK),
                                      blocked_r=u8(NK)),
                                 ["desc", "desc_r", "blocked", "blocked_r", "x3dc", "x3dr", "last_octave",
                                  "last_angle", "mp_desc"], ["desc", "desc_r", "mp_desc"]),
    "SearchByProjectionLocalStereo": (lambda: _matcher().SearchByProjectionLocalStereo,
                                      dict(params=plvi.LocalParams(), kps=kps(NK), desc=desc(NK), kps_r=kps(NK),
                                           desc_r=desc(NK), mp_flags=u8(NP), mp_proj=f32(NP, 4), mp_level=i32(NP),
                                           mp_proj_r=f32(NP, 4), mp_level_r=i32(NP), mp_desc=desc(NP),
                                           blocked=u8(NK), blocked_r=u8(NK), l2r=i32(NK), r2l=i32(NK)),
                                      ["desc", "desc_r", "blocked", "blocked_r", "l2r", "r2l", "mp_proj", "mp_level",
                                       "mp_proj_r", "mp_level_r", "mp_desc"], ["desc", "desc_r", "mp_desc"]),
    "SearchByProjectionKF": (lambda: _matcher().SearchByProjectionKF,
                             dict(params=plvi.RelocParams(), cur_kps=kps(NK), cur_desc=desc(NK), kf_flags=u8(NP),
                                  x3dc=f32(NP, 3), dist=f32(NP, 3), level=i32(NP), kf_angle=f32(NP),
                                  mp_desc=desc(NP), cur_blocked=u8(NK)),
                             ["cur_desc", "cur_blocked", "x3dc", "dist", "level", "kf_angle", "mp_desc"],
                             ["cur_desc", "mp_desc"]),
    "SearchByProjectionSim3": (lambda: _matcher().SearchByProjectionSim3,
                               dict(params=plvi.Sim3ProjParams(), kps=kps(NK), desc=desc(NK), matched=u8(NK),
                                    **POINTS),
                               ["desc", "matched", "x3dc", "dist", "dot", "level", "mp_desc"], ["desc", "mp_desc"]),
    "Fuse": (lambda: _matcher().Fuse,
             dict(params=plvi.FuseParams(), kps=kps(NK), desc=desc(NK), uright=f32(NK), **POINTS),
             ["desc", "uright", "x3dc", "dist", "dot", "level", "mp_desc"], ["desc", "mp_desc"]),
    "FuseSim3": (lambda: _matcher().FuseSim3, dict(params=plvi.FuseParams(), kps=kps(NK), desc=desc(NK), **POINTS),
                 ["desc", "x3dc", "dist", "dot", "level", "mp_desc"], ["desc", "mp_desc"]),
    "DescriptorDistance": (lambda: plvi.ORBmatcher.DescriptorDistance, dict(a=desc(NK), b=desc(NK)), ["b"],
                           ["a", "b"]),
    "LineMatcher.match": (lambda: plvi.LineMatcher.match, dict(desc1=desc(NK), desc2=desc(NP), nnr=0.9), [],
                          ["desc1", "desc2"]),
    "LineMatcher.matchNNR": (lambda: plvi.LineMatcher.matchNNR, dict(desc1=desc(NK), desc2=desc(NP), nnr=0.9), [],
                             ["desc1", "desc2"]),
    "LineMatcher.SearchByProjection": (lambda: plvi.LineMatcher.SearchByProjection,
                                       dict(params=plvi.LineProjParams(), cur_angle=f32(NK), cur_desc=desc(NK),
                                            grid=GRID, last_flags=u8(NP), last_x3dc=f32(NP, 6), last_octave=i32(NP),
                                            ml_desc=desc(NP), cur_blocked=u8(NK)),
                                       ["cur_desc", "cur_blocked", "last_x3dc", "last_octave", "ml_desc"],
                                       ["cur_desc", "ml_desc"]),
    "LineMatcher.Fuse": (lambda: plvi.LineMatcher.Fuse,
                         dict(params=plvi.FuseLineParams(), keylines=kls(NK), kl_desc=desc(NK), flags=u8(NP),
                              spc=f32(NP, 3), epc=f32(NP, 3), dist=f32(NP, 3), dot=arr(np.float64, NP), level=i32(NP),
                              ml_desc=desc(NP)),
                         ["kl_desc", "spc", "epc", "dist", "dot", "level", "ml_desc"], ["kl_desc", "ml_desc"]),
    "LineMatcher.SearchForTriangulation": (lambda: plvi.LineMatcher.SearchForTriangulation,
                                           dict(desc1=desc(NK), desc2=desc(NP), has_line1=u8(NK), has_line2=u8(NP)),
                                           ["has_line1", "has_line2"], ["desc1", "desc2"]),
    "LineMatcher.matchGrid": (lambda: plvi.LineMatcher.matchGrid,
                              dict(lines1=i32(NK, 4), desc1=desc(NK), grid=GRID, desc2=desc(NP),
                                   directions2=arr(np.float64, NP, 2)),
                              ["desc1", "directions2"], ["desc1", "desc2"]),
    "hamming_knn2": (lambda: plvi.hamming_knn2, dict(q=desc(NK), t=desc(NP)), [], ["q", "t"]),
    "ComputeStereoMatches": (lambda: plvi.ComputeStereoMatches,
                             dict(kpsL=kps(NK), descL=desc(NK), kpsR=kps(NP), descR=desc(NP), pyrL=PYR, pyrR=PYR,
                                  scale_factors=[1.0], inv_scale_factors=[1.0], mb=0.1, mbf=40.0),
                             ["descL", "descR"], ["descL", "descR"]),
    "ComputeStereoMatches_Lines": (lambda: plvi.ComputeStereoMatches_Lines,
                                   dict(klL=kls(NK), descL=desc(NK), klR=kls(NP), descR=desc(NP), klUn=kls(NK),
                                        width=64, height=48, mbf=40.0),
                                   ["descL", "descR", "klUn"], ["descL", "descR"]),
    "frustum_points": (lambda: plvi.frustum_points,
                       dict(params=plvi.FrustumParams(), pos=f32(NP, 3), normal=f32(NP, 3), dist=f32(NP, 2),
                            in_flags=u8(NP), proj=f32(NP, 4), level=i32(NP), depth=f32(NP)),
                       ["normal", "dist", "in_flags", "proj", "level", "depth"], []),
    "frustum_lines": (lambda: plvi.frustum_lines,
                      dict(params=plvi.FrustumParams(), sep=arr(np.float64, NP, 6), normal=f32(NP, 3),
                           dist=f32(NP, 2), in_flags=u8(NP), desc=desc(NP), proj=f32(NP, 4),
                           angle=arr(np.float64, NP)),
                      ["normal", "dist", "in_flags", "desc", "proj", "angle"], ["desc"]),
    "distinctive_descriptors": (lambda: plvi.distinctive_descriptors,
                                dict(pool=desc(NK), obs_off=i32(NP + 1), obs_row=i32(0)), [], ["pool"]),
    "search_for_initialization": (lambda: plvi.search_for_initialization,
                                  dict(kps1=kps(NK), desc1=desc(NK), prev_xy=f32(NK, 2), kps2=kps(NP),
                                       desc2=desc(NP)),
                                  ["desc1", "prev_xy", "desc2"], ["desc1", "desc2"]),
    "line_search_init": (lambda: plvi.line_search_init, dict(desc1=desc(NK), desc2=desc(NP)), [],
                         ["desc1", "desc2"]),
}

MUTATIONS = {"short": lambda a: a[:-1], "long": lambda a: np.concatenate([a, a[:1]]), "31 wide": lambda a: a[:, :31]}


def _params():
    for name, (_, _, companions, descs) in CASES.items():
        yield pytest.param(name, None, None, id=f"{name}-valid")
        for arg in companions:
            for how in ("short", "long"):
                yield pytest.param(name, arg, how, id=f"{name}-{arg}-{how}")
        for arg in descs:
            yield pytest.param(name, arg, "31 wide", id=f"{name}-{arg}-31wide")


@pytest.mark.parametrize("name, arg, how", _params())
def test_host_form_checks_its_tables(monkeypatch, name, arg, how):
    plvi.load()
    factory, kw, _, _ = CASES[name]
    fn = factory()

    def entered(entry, *args):
        if arg is None:
            raise Reached(entry)
        pytest.fail(f"{name}: {entry} entered with {arg} {how}")
    for mod, attr in ((plvi, "_call"), (plvi, "_status"), (_abi, "call"), (_abi, "status")):
        monkeypatch.setattr(mod, attr, entered)
    kw = dict(kw)
    if arg is None:
        with pytest.raises(Reached):
            fn(**kw)
        return
    kw[arg] = MUTATIONS[how](kw[arg])
    with pytest.raises(ValueError):
        fn(**kw)
