"""plvi — Python host mirror of the MI355X front end's C-ABI.

Thin ctypes layer over ``lib/libplvi_frontend.so`` (built from ``csrc/``).
Class and method names follow the reference interfaces they replace:

  ORBextractor  -> ORB_SLAM3::ORBextractor (include/ORBextractor.h:44-110)
  LineMatcher   -> ORB_SLAM3::LineMatcher  (include/LineMatcher.h:88-107)
  ORBmatcher    -> ORB_SLAM3::ORBmatcher   (include/ORBmatcher.h:39-78): SearchByBoW, SearchForTriangulation,
                   DescriptorDistance
  hamming_knn2  -> cv::BFMatcher(NORM_HAMMING).knnMatch(k=2) (LineMatcher.cpp:47-48)
  ORBVocabulary -> DBoW2::TemplatedVocabulary<FORB> (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h):
                   loadFromTextFile, transform(features, BowVector&, FeatureVector&, levelsup)
  KeyFrameDatabase -> ORB_SLAM3::KeyFrameDatabase (include/KeyFrameDatabase.h): add, erase, clearMap, clear,
                   DetectRelocalizationCandidates, DetectNBestCandidates

There is no CPU fallback: if the HIP library is missing or no GPU is
visible, construction raises.  PyTorch is only used by bench.py for device
memory and streams; this module needs numpy only.
"""
import ctypes
import os
import sys
import pathlib

import numpy as np

_PKG = pathlib.Path(__file__).resolve().parent.parent
# PLVI_LIB: an alternative build of the same library (A/B experiments, tools/build_variant.sh)
LIB_PATH = pathlib.Path(os.environ["PLVI_LIB"]) if os.environ.get("PLVI_LIB") else _PKG / "lib" / "libplvi_frontend.so"
HEADER_PATH = _PKG.parent / "include" / "plvi_frontend.h"

PLVI_OK = 0
PLVI_E_EMPTY = -1
PLVI_E_BADARG = -2
PLVI_E_CAPACITY = -3
PLVI_E_HIP = -4
PLVI_E_OVERFLOW = -5
PLVI_E_SIZE = -6
PLVI_E_CAPTURE = -7

# OpenCV-semantics switches (plvi_frontend.h PLVI_COMPAT_*)
COMPAT_GAUSS_ROUNDED = 1
COMPAT_RESIZE_V_GENERIC = 2
COMPAT_EXP_CV_TABLE = 4

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"),
                          ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"),
                          ("startPointY", "<f4"), ("endPointX", "<f4"), ("endPointY", "<f4"),
                          ("sPointInOctaveX", "<f4"), ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"),
                          ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"), ("numOfPixels", "<i4")])


class PlviError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed with status {code}")
        self.code = code


class GridParams(ctypes.Structure):
    """plvi_grid_params: mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv."""
    _fields_ = [("min_x", ctypes.c_float), ("min_y", ctypes.c_float), ("inv_w", ctypes.c_float),
                ("inv_h", ctypes.c_float)]


class Camera(ctypes.Structure):
    """plvi_camera: mK (fx, fy, cx, cy) and mDistCoef (k1, k2, p1, p2[, k3])."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("dist", ctypes.c_float * 5), ("ndist", ctypes.c_int)]

    @classmethod
    def make(cls, fx, fy, cx, cy, dist):
        c = cls()
        c.fx, c.fy, c.cx, c.cy = fx, fy, cx, cy
        for i, d in enumerate(dist):
            c.dist[i] = d
        c.ndist = len(dist)
        return c


def undistort_points(cam, xy):
    """cv::undistortPoints as Frame::UndistortKeyPoints calls it (src/Frame.cc:1124-1157): n x 2 float32."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    n = xy.shape[0]
    lib = load()
    d_in, d_out = DeviceBuffer(max(xy.nbytes, 8)), DeviceBuffer(max(xy.nbytes, 8))
    d_in.upload(xy)
    _check(lib.plvi_undistort_points(ctypes.byref(cam), ctypes.c_void_p(d_in.ptr), n, ctypes.c_void_p(d_out.ptr),
                                     None), "plvi_undistort_points")
    lib.plvi_device_synchronize()
    return d_out.download(np.zeros((n, 2), np.float32))


def image_bounds(cam, cols, rows):
    """Frame::ComputeImageBounds (src/Frame.cc:1199-1226): (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    b = np.zeros(4, np.float32)
    _check(load().plvi_image_bounds(ctypes.byref(cam), cols, rows, _ptr(b)), "plvi_image_bounds")
    return b


class ProjParams(ctypes.Structure):
    """plvi_proj_params (include/plvi_frontend.h)."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("mbf", ctypes.c_float), ("th", ctypes.c_float), ("min_x", ctypes.c_float),
                ("max_x", ctypes.c_float), ("min_y", ctypes.c_float), ("max_y", ctypes.c_float),
                ("inv_w", ctypes.c_float), ("inv_h", ctypes.c_float), ("forward", ctypes.c_int),
                ("backward", ctypes.c_int), ("check_orientation", ctypes.c_int), ("nlevels", ctypes.c_int),
                ("scale_factors", ctypes.c_float * 16)]


class InitParams(ctypes.Structure):
    """plvi_init_params (include/plvi_frontend.h): ORBmatcher::SearchForInitialization."""
    _fields_ = [("min_x", ctypes.c_float), ("min_y", ctypes.c_float), ("inv_w", ctypes.c_float),
                ("inv_h", ctypes.c_float), ("window", ctypes.c_int), ("nnratio", ctypes.c_float),
                ("check_orientation", ctypes.c_int)]


class TriangulationPair(ctypes.Structure):
    """plvi_triangulation_pair (include/plvi_frontend.h): the constants of one (KF1, KF2) pair of
    ORBmatcher::SearchForTriangulation."""
    _fields_ = [("F12", ctypes.c_float * 9), ("ep", ctypes.c_float * 2), ("n_sigma2", ctypes.c_int),
                ("sigma2", ctypes.c_float * 16), ("n_scale_factors", ctypes.c_int),
                ("scale_factors", ctypes.c_float * 16), ("only_stereo", ctypes.c_int), ("coarse", ctypes.c_int),
                ("check_orientation", ctypes.c_int)]

    @classmethod
    def make(cls, F12, ep, sigma2, scale_factors, only_stereo=False, coarse=False, check_orientation=True):
        t = cls()
        for i, v in enumerate(np.asarray(F12, np.float32).reshape(9)):
            t.F12[i] = v
        t.ep[0], t.ep[1] = float(ep[0]), float(ep[1])
        t.n_sigma2, t.n_scale_factors = len(sigma2), len(scale_factors)
        for i, v in enumerate(sigma2):
            t.sigma2[i] = v
        for i, v in enumerate(scale_factors):
            t.scale_factors[i] = v
        t.only_stereo, t.coarse, t.check_orientation = int(bool(only_stereo)), int(bool(coarse)), int(
            bool(check_orientation))
        return t


class LocalParams(ctypes.Structure):
    """plvi_local_params (include/plvi_frontend.h): ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>...)."""
    _fields_ = [("min_x", ctypes.c_float), ("min_y", ctypes.c_float), ("inv_w", ctypes.c_float),
                ("inv_h", ctypes.c_float), ("th", ctypes.c_float), ("nnratio", ctypes.c_float),
                ("nlevels", ctypes.c_int), ("scale_factors", ctypes.c_float * 16)]


class RelocParams(ctypes.Structure):
    """plvi_reloc_params (include/plvi_frontend.h): ORBmatcher::SearchByProjection(Frame&, KeyFrame*,
    sAlreadyFound, th, ORBdist)."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float), ("inv_w", ctypes.c_float), ("inv_h", ctypes.c_float),
                ("th", ctypes.c_float), ("orb_dist", ctypes.c_int), ("check_orientation", ctypes.c_int),
                ("nlevels", ctypes.c_int), ("scale_factors", ctypes.c_float * 16)]


class Sim3ProjParams(ctypes.Structure):
    """plvi_sim3_proj_params (include/plvi_frontend.h): ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints,
    [vpPointsKFs,] vpMatched, [vpMatchedKF,] th, ratioHamming); projection 0 / 1 = the :473 / :588 overload."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float), ("inv_w", ctypes.c_float), ("inv_h", ctypes.c_float),
                ("th", ctypes.c_int), ("ratio_hamming", ctypes.c_float), ("projection", ctypes.c_int),
                ("nlevels", ctypes.c_int), ("scale_factors", ctypes.c_float * 16)]


class FuseParams(ctypes.Structure):
    """plvi_fuse_params (include/plvi_frontend.h): the two ORBmatcher::Fuse overloads; mode 0 / 1 = Fuse(pKF,
    vpMapPoints, th) / Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float), ("inv_w", ctypes.c_float), ("inv_h", ctypes.c_float),
                ("th", ctypes.c_float), ("bf", ctypes.c_float), ("mode", ctypes.c_int), ("nlevels", ctypes.c_int),
                ("scale_factors", ctypes.c_float * 16), ("inv_level_sigma2", ctypes.c_float * 16)]


class FuseLineParams(ctypes.Structure):
    """plvi_fuse_line_params (include/plvi_frontend.h): LineMatcher::Fuse."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float), ("th", ctypes.c_float), ("nlevels", ctypes.c_int),
                ("scale_factors", ctypes.c_float * 16)]


FUSE_CHUNK = 64  # PLVI_FUSE_CHUNK: candidates per workgroup of the two Fuse kernels
DISTINCTIVE_MAX_OBS = 2048  # PLVI_DISTINCTIVE_MAX_OBS: longest observation list of distinctive_descriptors
KFDB_MAX_WORDS = 8192       # PLVI_KFDB_MAX_WORDS: longest BowVector of a KeyFrameDatabase slot or query
KFDB_NEIGHBOURS = 10        # PLVI_KFDB_NEIGHBOURS: row length of the covisibility table


class LineProjParams(ctypes.Structure):
    """plvi_line_proj_params (include/plvi_frontend.h): LineMatcher::SearchByProjection."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float), ("inv_w", ctypes.c_double), ("inv_h", ctypes.c_double),
                ("th", ctypes.c_float), ("angth", ctypes.c_float), ("grid_cols", ctypes.c_int),
                ("grid_rows", ctypes.c_int), ("range_hint", ctypes.c_int), ("nlevels", ctypes.c_int),
                ("scale_l", ctypes.c_float * 8)]


class FrustumCamera(ctypes.Structure):
    """plvi_frustum_camera (include/plvi_frontend.h): one camera of a frame for the frustum tests."""
    _fields_ = [("R", ctypes.c_float * 9), ("t", ctypes.c_float * 3), ("O", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("kb", ctypes.c_float * 4), ("model", ctypes.c_int)]


class FrustumParams(ctypes.Structure):
    """plvi_frustum_params (include/plvi_frontend.h): Frame::isInFrustum / isInFrustum_l of one frame."""
    _fields_ = [("cam", FrustumCamera * 2), ("two_camera", ctypes.c_int), ("mbf", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float), ("view_cos_limit", ctypes.c_float), ("far_points", ctypes.c_int),
                ("far_th", ctypes.c_float), ("nlevels", ctypes.c_int), ("log_scale_factor", ctypes.c_float),
                ("level_ratio", ctypes.c_float * 16), ("compat", ctypes.c_uint)]


FRUSTUM_SEARCH, FRUSTUM_OBS, FRUSTUM_SEARCH_R, FRUSTUM_VISIBLE, FRUSTUM_TRACK = 1, 2, 4, 8, 16


def _same_len(n, **arrays):
    """The C entry points read n records from every host array: refuse a shorter (or longer) one
    instead of letting hipMemcpy read past its end."""
    for name, a in arrays.items():
        if a is not None and len(a) != n:
            raise ValueError(f"{name} has {len(a)} records, expected {n}")


def frustum_params_init(p):
    """plvi_frustum_params_init: PredictScale's level_ratio table from nlevels / log_scale_factor."""
    _check(load().plvi_frustum_params_init(ctypes.byref(p)), "plvi_frustum_params_init")
    return p


def frustum_points(params, pos, normal, dist, in_flags, proj=None, level=None, depth=None, proj_r=None,
                   level_r=None):
    """Frame::isInFrustum over one frame's local MapPoints (src/Frame.cc:758-847) from host memory.
    proj / level / depth (/ proj_r / level_r) are the MapPoint fields on entry (stale values are kept
    where the reference keeps them).  Returns (nToMatch, flags, proj, level, depth, proj_r, level_r)."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    nr = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    ds = np.ascontiguousarray(dist, np.float32).reshape(-1, 2)
    fi = np.ascontiguousarray(in_flags, np.uint8)
    pr = np.zeros((n, 4), np.float32) if proj is None else np.array(proj, np.float32).reshape(-1, 4)
    lv = np.zeros(n, np.int32) if level is None else np.array(level, np.int32)
    de = np.zeros(n, np.float32) if depth is None else np.array(depth, np.float32)
    two = bool(params.two_camera)
    prr = (np.zeros((n, 4), np.float32) if proj_r is None else np.array(proj_r, np.float32).reshape(-1, 4)) \
        if two else None
    lvr = (np.zeros(n, np.int32) if level_r is None else np.array(level_r, np.int32)) if two else None
    _same_len(n, normal=nr, dist=ds, in_flags=fi, proj=pr, level=lv, depth=de, proj_r=prr, level_r=lvr)
    fo = np.zeros(max(n, 1), np.uint8)
    nv = _check(load().plvi_frustum_points(ctypes.byref(params), _ptr(pos), _ptr(nr), _ptr(ds), _ptr(fi), n,
                                           _ptr(fo), _ptr(pr), _ptr(lv), None if prr is None else _ptr(prr),
                                           None if lvr is None else _ptr(lvr), _ptr(de)), "plvi_frustum_points")
    return nv, fo[:n], pr, lv, de, prr, lvr


def frustum_lines(params, sep, normal, dist, in_flags, desc=None, proj=None, angle=None):
    """Frame::isInFrustum_l over one frame's local MapLines (src/Frame.cc:849-933) from host memory.
    Returns (inview, proj, angle, compact, compact_desc): compact = mvpLocalMapLines_InFrustum as local
    indices, compact_desc = their descriptors (None without desc)."""
    sp = np.ascontiguousarray(sep, np.float64).reshape(-1, 6)
    n = len(sp)
    nr = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    ds = np.ascontiguousarray(dist, np.float32).reshape(-1, 2)
    fi = np.ascontiguousarray(in_flags, np.uint8)
    de = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    pr = np.zeros((n, 4), np.float32) if proj is None else np.array(proj, np.float32).reshape(-1, 4)
    an = np.zeros(n, np.float64) if angle is None else np.array(angle, np.float64)
    _same_len(n, normal=nr, dist=ds, in_flags=fi, desc=de, proj=pr, angle=an)
    iv = np.zeros(max(n, 1), np.uint8)
    cp = np.zeros(max(n, 1), np.int32)
    cd = np.zeros((max(n, 1), 32), np.uint8)
    nc = _check(load().plvi_frustum_lines(ctypes.byref(params), _ptr(sp), _ptr(nr), _ptr(ds), _ptr(fi),
                                          None if de is None else _ptr(de), n, _ptr(iv), _ptr(pr), _ptr(an),
                                          _ptr(cp), _ptr(cd)), "plvi_frustum_lines")
    return iv[:n], pr, an, cp[:nc], (None if de is None else cd[:nc])


def grid_geometry(width, height):
    """Frame ctor grid geometry without distortion (mnMinX = 0, mnMaxX = cols, ...;
    Frame.cc:156-157): (min_x, max_x, min_y, max_y, inv_w, inv_h) as float32."""
    f = np.float32
    return (f(0), f(width), f(0), f(height), f(64) / (f(width) - f(0)), f(48) / (f(height) - f(0)))


class OrbParams(ctypes.Structure):
    _fields_ = [("nfeatures", ctypes.c_int), ("scale_factor", ctypes.c_float), ("nlevels", ctypes.c_int),
                ("ini_th_fast", ctypes.c_int), ("min_th_fast", ctypes.c_int), ("compat", ctypes.c_uint)]


class LineParams(ctypes.Structure):
    _fields_ = [("nfeatures", ctypes.c_int), ("refine", ctypes.c_int), ("lsd_scale", ctypes.c_float),
                ("nlevels", ctypes.c_int), ("scale", ctypes.c_float), ("extractor", ctypes.c_int),
                ("compat", ctypes.c_uint)]


_lib = None
_runtime = None

c_int_p = ctypes.POINTER(ctypes.c_int)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)


def _declare(lib):
    V, I, S, F, P = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, c_int_p
    sig = {
        "plvi_version": ([], ctypes.c_char_p),
        "plvi_device_count": ([], I),
        "plvi_orb_create": ([ctypes.POINTER(OrbParams), I, I, I, I, c_void_pp], I),
        "plvi_orb_destroy": ([V], I),
        "plvi_orb_extract": ([V, V, I, I, S, I, I, V, V, I, P, P], I),
        "plvi_orb_extract_batch": ([V, V, I, S, S, I, I, V], I),
        "plvi_orb_outputs": ([V, c_void_pp, c_void_pp, c_void_pp, c_void_pp, P], I),
        "plvi_orb_errors": ([V, V, P, V], I),
        "plvi_lines_errors": ([V, V, P, V], I),
        "plvi_lines_kernel_timing": ([V, I], I),
        "plvi_lines_kernel_timing_read": ([V, V, P], I),
        "plvi_lines_kernel_timing_read_kind": ([V, I, V, P], I),
        "plvi_line_match_nnr_inout": ([V, I, V, I, F, V, I], I),
        "plvi_line_match_inout": ([V, I, V, I, F, V, I], I),
        "plvi_orb_pyramid_level": ([V, I, I, V, P, P], I),
        "plvi_orb_pyramid_device": ([V, I, c_void_pp, ctypes.POINTER(S), P, P, P], I),
        "plvi_orb_scale_tables": ([V, V, V, V, V], I),
        "plvi_orb_level_quota": ([V, V], I),
        "plvi_orb_profile": ([V, I], I),
        "plvi_orb_profile_read": ([V, V, P], I),
        "plvi_orb_kernel_timing": ([V, I], I),
        "plvi_orb_kernel_timing_read": ([V, V, P], I),
        "plvi_orb_kernel_timing_read_kind": ([V, I, V, P], I),
        "plvi_orb_debug_node_cap": ([V, I], I),
        "plvi_hamming_knn2_batch": ([V, V, I, V, V, I, I, V, V, V, V, V], I),
        "plvi_hamming_knn2": ([V, I, V, I, V, V, V, V], I),
        "plvi_line_match_nnr": ([V, I, V, I, F, V], I),
        "plvi_line_match": ([V, I, V, I, F, V], I),
        "plvi_line_match_batch": ([V, V, I, V, V, I, I, F, V, V, V, V], I),
        "plvi_lines_create": ([ctypes.POINTER(LineParams), I, I, I, I, c_void_pp], I),
        "plvi_lines_destroy": ([V], I),
        "plvi_lines_extract": ([V, V, I, I, S, V, V, V, I, P], I),
        "plvi_lines_extract_batch": ([V, V, I, S, S, V], I),
        "plvi_lines_outputs": ([V, c_void_pp, c_void_pp, c_void_pp, c_void_pp, P], I),
        "plvi_lines_pyramid_level": ([V, I, I, V, P, P], I),
        "plvi_lines_scale_tables": ([V, V, V, V, V], I),
        "plvi_lines_profile": ([V, I], I),
        "plvi_lines_profile_read": ([V, V, P], I),
        "plvi_lines_debug_stats": ([V, V], I),
        "plvi_lines_debug_mw_stats": ([V, V], I),
        "plvi_lines_debug_planes": ([V, I, I, V, V, V, P, P], I),
        "plvi_lines_debug_sobel": ([V, I, I, V, P, P], I),
        "plvi_lines_debug_raw_lines": ([V, I, I, V, I, P], I),
        "plvi_descriptor_distance_batch": ([V, V, I, I, V, V], I),
        "plvi_search_by_bow": ([F, I, V, V, V, I, V, V, I, V, V, V, I, V, V, I, V, V], I),
        "plvi_search_by_bow_stereo": ([F, I, V, V, V, I, V, V, I, V, V, V, I, V, V, I, V, I, V], I),
        "plvi_search_by_bow_stereo_batch": ([I, F, I, I, I, I, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V,
                                             V], I),
        "plvi_search_by_bow_batch": ([I, F, I, I, I, I, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V], I),
        "plvi_line_match_grid": ([V, V, I, I, I, V, V, V, V, I, I, I, I, I, I, V], I),
        "plvi_line_match_grid_batch": ([I, V, V, V, I, I, I, V, V, I, V, V, V, I, I, I, I, I, I, V, V, V, V], I),
        "plvi_frame_extract_batch": ([V, V, V, I, S, S, I, I, V], I),
        "plvi_assign_grid_batch": ([V, V, I, I, V, V, V, V], I),
        "plvi_undistort_points": ([V, V, I, V, V], I),
        "plvi_undistort_keypoints_batch": ([V, V, V, I, I, V, V], I),
        "plvi_undistort_keylines_batch": ([V, V, V, I, I, V, V], I),
        "plvi_image_bounds": ([V, I, I, V], I),
        "plvi_search_by_projection_batch": ([I, V, V, V, V, I, V, V, V, V, V, V, V, V, V, V, I, V, V, V], I),
        "plvi_search_by_projection": ([V, V, V, I, V, V, V, V, V, V, V, I, V], I),
        "plvi_stereo_frame_extract_batch": ([V, V, V, V, V, V, I, S, S, I, I, V], I),
        "plvi_event_create": ([c_void_pp], I),
        "plvi_event_record": ([V, V], I),
        "plvi_stream_wait_event": ([V, V], I),
        "plvi_event_destroy": ([V], I),
        "plvi_frame_orb_event": ([V, c_void_pp], I),
        "plvi_frame_extract_match_batch": ([V, V, V, I, S, S, I, I, V, V, V, V, F, V, V, V, V], I),
        "plvi_stream_create": ([c_void_pp], I),
        "plvi_stream_destroy": ([V], I),
        "plvi_stream_synchronize": ([V], I),
        "plvi_search_for_initialization_batch": ([I, V, V, V, V, I, V, V, V, V, I, V, V, V, V, V], I),
        "plvi_line_search_init_batch": ([V, V, I, V, V, I, I, V, V, V, V, V], I),
        "plvi_line_search_triangulation_batch": ([V, V, I, V, V, I, I, V, V, V, V, V, V, V], I),
        "plvi_search_for_triangulation_batch": ([I, V, I, I, I, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V,
                                                 V, V, V], I),
        "plvi_search_for_triangulation": ([V, V, V, I, V, V, I, V, V, V, V, V, I, V, V, I, V, V, V, V], I),
        "plvi_search_by_bow_kf_batch": ([I, F, I, I, I, I, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V], I),
        "plvi_search_by_bow_kf": ([F, I, V, V, V, I, V, V, I, V, V, V, V, I, V, V, I, V, V], I),
        "plvi_search_sim3_projection_batch": ([I, V, V, V, V, I, V, V, V, V, V, V, V, V, V, V, I, V, V, V], I),
        "plvi_search_sim3_projection": ([V, V, V, I, V, V, V, V, V, V, V, I, V], I),
        "plvi_fuse_points_batch": ([I, V, V, V, V, I, V, V, V, V, V, V, V, V, V, V, I, V, V, V, V], I),
        "plvi_fuse_points": ([V, V, V, I, V, V, V, V, V, V, V, I, V, V], I),
        "plvi_fuse_lines_batch": ([I, V, V, V, V, I, V, V, V, V, V, V, V, V, I, V, V, V, V], I),
        "plvi_fuse_lines": ([V, V, V, I, V, V, V, V, V, V, V, I, V, V], I),
        "plvi_distinctive_descriptors_batch": ([I, V, I, V, V, I, V, V, V, V], I),
        "plvi_distinctive_descriptors": ([V, I, V, V, I, V, V, V], I),
        "plvi_kfdb_create": ([I, I, I, I, I, c_void_pp], I),
        "plvi_kfdb_destroy": ([V], I),
        "plvi_kfdb_add_batch": ([V, I, V, V, V, V, I, V], I),
        "plvi_kfdb_add": ([V, I, I, V, V, I], I),
        "plvi_kfdb_erase": ([V, I, V, V], I),
        "plvi_kfdb_clear_map": ([V, I, V], I),
        "plvi_kfdb_clear": ([V, V], I),
        "plvi_kfdb_errors": ([V, P, V], I),
        "plvi_kfdb_query_batch": ([V, I, V, V, V, I, V, I, I, V, V, V, V, I, V, V, V, V, V, I, V, V, V, V, V, V], I),
        "plvi_kfdb_query": ([V, V, V, I, I, I, I, V, I, V, V, I, V, I, V, P, V, P], I),
        "plvi_search_local_batch": ([I, V, V, V, V, I, V, V, V, V, V, V, V, V, V, I, V, V, V], I),
        "plvi_search_local": ([V, V, V, I, V, V, V, V, V, V, I, V], I),
        "plvi_search_by_projection_stereo_batch": ([I, V, V, V, V, V, I, V, V, V, V, V, V, I, V, V, V, V, V, V, V, V,
                                                    V, V, I, V, V, V, V], I),
        "plvi_search_by_projection_stereo": ([V, V, V, V, I, V, V, V, I, V, V, V, V, V, V, V, I, V, V], I),
        "plvi_search_local_stereo_batch": ([I, V, V, V, V, I, V, V, V, V, V, V, V, I, V, V, V, V, V, V, V, V, V, V,
                                            V, I, V, V, V, V], I),
        "plvi_search_local_stereo": ([V, V, V, I, V, V, V, V, I, V, V, V, V, V, V, V, V, I, V, V], I),
        "plvi_search_reloc_batch": ([I, V, V, V, V, I, V, V, V, V, V, V, V, V, V, V, I, V, V, V], I),
        "plvi_search_reloc": ([V, V, V, I, V, V, V, V, V, V, V, I, V], I),
        "plvi_line_search_projection_batch": ([I, V, V, V, V, V, I, V, V, I, V, V, V, V, V, I, V, V, V, V], I),
        "plvi_line_search_projection": ([V, V, V, V, I, V, V, V, V, V, V, I, V], I),
        "plvi_vocab_load_text": ([ctypes.c_char_p, I, I, c_void_pp], I),
        "plvi_vocab_create": ([I, I, I, I, I, V, V, V, V, I, c_void_pp], I),
        "plvi_vocab_destroy": ([V], I),
        "plvi_vocab_info": ([V, V], I),
        "plvi_vocab_transform": ([V, V, I, I, V, V, P, V, V, V, P], I),
        "plvi_vocab_transform_features": ([V, V, I, I, V, V], I),
        "plvi_vocab_transform_batch": ([V, V, V, I, I, I, V, V, V, V, V, V, V, V, V, V], I),
        "plvi_stereo_match_batch": ([V, V, I, F, F, V, V, V, V, V], I),
        "plvi_stereo_match": ([V, V, I, V, V, I, I, V, V, V, V, V, V, V, F, F, V, V], I),
        "plvi_stereo_lines_scratch_bytes": ([I, I, I, I], S),
        "plvi_stereo_lines_batch": ([I, V, V, V, I, V, V, V, I, V, I, I, F, I, I, V, S, V, V, V, V, V, V, V], I),
        "plvi_stereo_lines": ([V, V, I, V, V, I, V, I, I, F, I, V, V, V, V], I),
        "plvi_frustum_params_init": ([V], I),
        "plvi_frustum_points_batch": ([I, V, V, V, V, V, V, I, V, V, V, V, V, V, V, V], I),
        "plvi_frustum_points": ([V, V, V, V, V, I, V, V, V, V, V, V], I),
        "plvi_frustum_lines_batch": ([I, V, V, V, V, V, V, V, I, V, V, V, V, V, V, V], I),
        "plvi_frustum_lines": ([V, V, V, V, V, V, I, V, V, V, V, V], I),
        "plvi_local_lines_filter_batch": ([I, V, V, V, V, I, V, V, V, V, I, V, V, V, V], I),
        "plvi_local_map_scratch_bytes": ([I, I, I, I], S),
        "plvi_local_map_batch": ([I, V, V, V, V, V, V, S, V], I),
        "plvi_local_map": ([V, V, V, V, V], I),
        "plvi_covis_create": ([I, I, I, c_void_pp], I),
        "plvi_covis_destroy": ([V], I),
        "plvi_covis_scratch_bytes": ([I, I], S),
        "plvi_covis_update_batch": ([V, I, V, V, V, V, V, V, S, V], I),
        "plvi_covis_erase_batch": ([V, I, V, V, V, I, V, V], I),
        "plvi_covis_resort_batch": ([V, I, V, V, V, I, V, V], I),
        "plvi_covis_by_weight_batch": ([V, I, V, V, V, V], I),
        "plvi_covis_weight_batch": ([V, I, V, V, V, V], I),
        "plvi_covis_rows": ([V, c_void_pp, c_void_pp, c_void_pp, P], I),
        "plvi_covis_download": ([V, I, V, V, P, V, V, P, P], I),
        "plvi_covis_update": ([V, I, V, V, V, V], I),
        "plvi_device_malloc": ([c_void_pp, S], I),
        "plvi_device_free": ([V], I),
        "plvi_memcpy": ([V, V, S, I], I),
        "plvi_memcpy_async": ([V, V, S, I, V], I),
        "plvi_device_synchronize": ([], I),
        "plvi_graph_capture_begin": ([V], I),
        "plvi_graph_capture_end": ([V, c_void_pp], I),
        "plvi_graph_launch": ([V, V], I),
        "plvi_graph_destroy": ([V], I),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return lib


def load(runtime=None):
    """Load the HIP library (raises if it was not built: there is no fallback).

    Which HIP runtime the library binds to is decided here, once per process:
    PyTorch's bundled libamdhip64 (HIP 7.0 on this image) and /opt/rocm's
    (7.2) share the SONAME libamdhip64.so.7, so whichever loads first serves
    both -- unless ours comes first and torch is imported later, in which case
    torch loads its own copy by file name and that second runtime finds no
    device.  `runtime`:

    * "torch": import torch first (one runtime for both).  On the 7.0 runtime
      `plvi_frame_extract_batch` / `plvi_stereo_frame_extract_batch` refuse
      stream capture with PLVI_E_CAPTURE; everything else
      behaves identically.
    * "system": do not import torch; the library binds to /opt/rocm's runtime
      (capture supported).  Do not import torch later in the same process.
    * None (default): "torch" if torch is already imported, else the
      PLVI_RUNTIME environment variable ("torch" / "system"; PLVI_NO_TORCH=1
      means "system"), else "torch" when torch is installed -- the safe choice
      for a process that may import torch later.
    """
    global _lib, _runtime
    if _lib is None:
        if runtime is None:
            if "torch" in sys.modules:
                runtime = "torch"
            elif os.environ.get("PLVI_NO_TORCH"):
                runtime = "system"
            else:
                runtime = os.environ.get("PLVI_RUNTIME", "torch")
        if runtime not in ("torch", "system"):
            raise ValueError(f"plvi.load: runtime must be 'torch' or 'system', not {runtime!r}")
        if runtime == "torch":
            try:
                import torch  # noqa: F401
            except ImportError:
                runtime = "system"
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} missing: build it with `make -C pl-vi-orbslam3_amd`")
        _lib = _declare(ctypes.CDLL(str(LIB_PATH)))
        _runtime = runtime
    elif runtime is not None and runtime != _runtime:
        raise RuntimeError(f"plvi.load: library already bound to the {_runtime!r} HIP runtime")
    return _lib


def bound_runtime():
    """'torch' or 'system': the HIP runtime the loaded library is bound to (None before load())."""
    return _runtime


def exported_symbols():
    """Function names declared in include/plvi_frontend.h."""
    import re
    txt = HEADER_PATH.read_text()
    return sorted(set(re.findall(r"\b(plvi_[a-z0-9_]+)\s*\(", txt)))


class DeviceBuffer:
    """hipMalloc'd buffer owned from Python (no torch needed)."""

    def __init__(self, nbytes):
        self._lib = load()
        p = ctypes.c_void_p()
        _check(self._lib.plvi_device_malloc(ctypes.byref(p), max(1, nbytes)), "plvi_device_malloc")
        self.ptr, self.nbytes = p.value, nbytes

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(self._lib.plvi_memcpy(ctypes.c_void_p(self.ptr), _ptr(arr), arr.nbytes, 1), "plvi_memcpy")

    def download(self, arr, src_ptr=None):
        _check(self._lib.plvi_memcpy(_ptr(arr), ctypes.c_void_p(src_ptr or self.ptr), arr.nbytes, 2),
               "plvi_memcpy")
        return arr

    def __del__(self):
        try:
            if self.ptr:
                self._lib.plvi_device_free(ctypes.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def download(ptr, arr):
    """Copy device memory at `ptr` into numpy array `arr` (synchronous)."""
    _check(load().plvi_memcpy(_ptr(arr), ctypes.c_void_p(ptr), arr.nbytes, 2), "plvi_memcpy")
    return arr


def _check(rc, what):
    if rc < 0:
        raise PlviError(rc, what)
    return rc


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class ORBextractor:
    """ORB_SLAM3::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST).

    ``extractor(image, mask, vLappingArea)`` returns ``(monoIndex, keypoints,
    descriptors)`` like operator() (src/ORBextractor.cc:1068): keypoints is a
    structured array in cv::KeyPoint layout, descriptors an N x 32 uint8 array.
    An empty image returns ``(-1, empty, empty)``.
    """

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width=640, height=480,
                 max_batch=1, device=0, compat=0):
        self._lib = load()
        self.params = OrbParams(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, compat)
        self.width, self.height, self.max_batch = width, height, max_batch
        self.nlevels = nlevels
        h = ctypes.c_void_p()
        _check(self._lib.plvi_orb_create(ctypes.byref(self.params), width, height, max_batch, device,
                                         ctypes.byref(h)), "plvi_orb_create")
        self._h = h
        cap = ctypes.c_int()
        self._lib.plvi_orb_outputs(self._h, None, None, None, None, ctypes.byref(cap))
        self.kp_cap = cap.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.plvi_orb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __call__(self, image, mask=None, vLappingArea=(0, 0)):
        """operator(): any frame size (a new size re-plans the handle); an
        empty image returns (-1, empty, empty) from the C-ABI's PLVI_E_EMPTY."""
        image = np.ascontiguousarray(image if image is not None else np.zeros((0, 0)), dtype=np.uint8)
        h, w = image.shape if image.ndim == 2 else (0, 0)
        if (w, h) != (self.width, self.height) and w > 0 and h > 0:
            self.width, self.height = w, h
        kps = np.zeros(self.kp_cap, KEYPOINT_DTYPE)
        desc = np.zeros((self.kp_cap, 32), np.uint8)
        n, mono = ctypes.c_int(), ctypes.c_int()
        rc = self._lib.plvi_orb_extract(self._h, _ptr(image) if image.size else None, w, h, w,
                                        int(vLappingArea[0]), int(vLappingArea[1]), _ptr(kps), _ptr(desc),
                                        self.kp_cap, ctypes.byref(n), ctypes.byref(mono))
        if rc == PLVI_E_EMPTY:
            return -1, np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
        if rc == PLVI_E_CAPACITY:  # a re-planned (larger) frame: grow the host buffers once
            self._refresh_cap()
            return self(image, mask, vLappingArea)
        _check(rc, "plvi_orb_extract")
        self._refresh_cap()
        return mono.value, kps[:n.value].copy(), desc[:n.value].copy()

    def _refresh_cap(self):
        cap = ctypes.c_int()
        self._lib.plvi_orb_outputs(self._h, None, None, None, None, ctypes.byref(cap))
        self.kp_cap = cap.value

    def errors(self, stream=None, per_frame=False):
        """Read-and-clear device error flags of the batches run so far (PLVI_FERR_*)."""
        flags = np.zeros(self.max_batch, np.int32)
        anyf = ctypes.c_int()
        _check(self._lib.plvi_orb_errors(self._h, _ptr(flags), ctypes.byref(anyf), ctypes.c_void_p(stream or 0)),
               "plvi_orb_errors")
        return flags if per_frame else anyf.value

    # --- batched device path (bench / multi-frame) ---------------------------
    def extract_batch(self, d_frames_ptr, n_frames, frame_stride, row_stride, lap=(0, 0), stream=None):
        _check(self._lib.plvi_orb_extract_batch(self._h, ctypes.c_void_p(d_frames_ptr), n_frames, frame_stride,
                                                row_stride, lap[0], lap[1], ctypes.c_void_p(stream or 0)),
               "plvi_orb_extract_batch")

    def outputs(self):
        """Device pointers (kps, desc, count, mono) and per-frame capacity."""
        kp, de, co, mo = (ctypes.c_void_p() for _ in range(4))
        cap = ctypes.c_int()
        _check(self._lib.plvi_orb_outputs(self._h, ctypes.byref(kp), ctypes.byref(de), ctypes.byref(co),
                                          ctypes.byref(mo), ctypes.byref(cap)), "plvi_orb_outputs")
        return kp.value, de.value, co.value, mo.value, cap.value

    ORB_STAGES = ("level", "nms", "sat", "octree", "best", "describe", "assemble")

    def profile(self, enable=True):
        _check(self._lib.plvi_orb_profile(self._h, int(enable)), "plvi_orb_profile")

    def profile_read(self):
        ms = np.zeros(7, np.float32)
        runs = ctypes.c_int()
        _check(self._lib.plvi_orb_profile_read(self._h, _ptr(ms), ctypes.byref(runs)), "plvi_orb_profile_read")
        return dict(zip(self.ORB_STAGES, ms.tolist())), runs.value

    def kernel_timing(self, enable=True):
        """Event pair around every blur + FAST and pyramid kernel launch (rooflines)."""
        _check(self._lib.plvi_orb_kernel_timing(self._h, int(enable)), "plvi_orb_kernel_timing")

    def kernel_timing_read(self, kind=0):
        """(total ms, launches) since kernel_timing(True): kind 0 = orb_blur_fast_kernel, 1 = orb_pyramid_kernel."""
        tot = ctypes.c_float()
        n = ctypes.c_int()
        _check(self._lib.plvi_orb_kernel_timing_read_kind(self._h, int(kind), ctypes.byref(tot), ctypes.byref(n)),
               "plvi_orb_kernel_timing_read_kind")
        return tot.value, n.value

    # --- reference getters ---------------------------------------------------
    def _tables(self):
        out = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        _check(self._lib.plvi_orb_scale_tables(self._h, *[_ptr(a) for a in out]), "plvi_orb_scale_tables")
        return out

    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return float(np.float32(self.params.scale_factor))

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def level_quota(self):
        q = np.zeros(self.nlevels, np.int32)
        _check(self._lib.plvi_orb_level_quota(self._h, _ptr(q)), "plvi_orb_level_quota")
        return q

    def pyramid_level(self, level, frame=0):
        """mvImagePyramid[level] of the last call (lazy D2H)."""
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.plvi_orb_pyramid_level(self._h, frame, level, None, ctypes.byref(w), ctypes.byref(h)),
               "plvi_orb_pyramid_level")
        out = np.zeros((h.value, w.value), np.uint8)
        _check(self._lib.plvi_orb_pyramid_level(self._h, frame, level, _ptr(out), None, None),
               "plvi_orb_pyramid_level")
        return out

    @property
    def mvImagePyramid(self):
        return [self.pyramid_level(l) for l in range(self.nlevels)]

    def pyramid_device(self, level):
        """Device view of mvImagePyramid[level]: (frame-0 pointer, frame stride, w, h)."""
        p, fs = ctypes.c_void_p(), ctypes.c_size_t()
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.plvi_orb_pyramid_device(self._h, level, ctypes.byref(p), ctypes.byref(fs), ctypes.byref(w),
                                                 ctypes.byref(h), None), "plvi_orb_pyramid_device")
        return p.value, fs.value, w.value, h.value


class Lineextractor:
    """ORB_SLAM3::Lineextractor(lsd_nfeatures, lsd_refine, lsd_scale, nlevels, scale, extractor).

    ``extractor(image, mask)`` returns ``(keylines, descriptors, keylineFunctions)``
    as operator() fills them (src/LineExtractor.cc:45-117): keylines in KeyLine
    layout, n x 32 LBD descriptors, n x 3 normalised line equations.
    """

    STAGES = ("pyramid", "lsd_prep", "region_grow", "assemble", "lbd")

    def __init__(self, lsd_nfeatures, lsd_refine, lsd_scale, nlevels, scale, extractor=0, width=640, height=480,
                 max_batch=1, device=0, compat=0):
        self._lib = load()
        self.params = LineParams(lsd_nfeatures, lsd_refine, lsd_scale, nlevels, scale, extractor, compat)
        self.width, self.height, self.max_batch, self.nlevels = width, height, max_batch, nlevels
        h = ctypes.c_void_p()
        _check(self._lib.plvi_lines_create(ctypes.byref(self.params), width, height, max_batch, device,
                                           ctypes.byref(h)), "plvi_lines_create")
        self._h = h
        cap = ctypes.c_int()
        self._lib.plvi_lines_outputs(self._h, None, None, None, None, ctypes.byref(cap))
        self.cap = cap.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.plvi_lines_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __call__(self, image, mask=None):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape
        kl = np.zeros(self.cap, KEYLINE_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        fn = np.zeros((self.cap, 3), np.float64)
        n = ctypes.c_int()
        _check(self._lib.plvi_lines_extract(self._h, _ptr(image), w, h, w, _ptr(kl), _ptr(desc), _ptr(fn), self.cap,
                                            ctypes.byref(n)), "plvi_lines_extract")
        self.width, self.height = w, h
        k = n.value
        return kl[:k].copy(), desc[:k].copy(), fn[:k].copy()

    def errors(self, stream=None, per_frame=False):
        """Read-and-clear device error flags of the batches run so far (PLVI_FERR_*)."""
        flags = np.zeros(self.max_batch, np.int32)
        anyf = ctypes.c_int()
        _check(self._lib.plvi_lines_errors(self._h, _ptr(flags), ctypes.byref(anyf), ctypes.c_void_p(stream or 0)),
               "plvi_lines_errors")
        return flags if per_frame else anyf.value

    def extract_batch(self, d_frames_ptr, n_frames, frame_stride, row_stride, stream=None):
        _check(self._lib.plvi_lines_extract_batch(self._h, ctypes.c_void_p(d_frames_ptr), n_frames, frame_stride,
                                                  row_stride, ctypes.c_void_p(stream or 0)),
               "plvi_lines_extract_batch")

    def outputs(self):
        kl, de, fn, co = (ctypes.c_void_p() for _ in range(4))
        cap = ctypes.c_int()
        _check(self._lib.plvi_lines_outputs(self._h, ctypes.byref(kl), ctypes.byref(de), ctypes.byref(fn),
                                            ctypes.byref(co), ctypes.byref(cap)), "plvi_lines_outputs")
        return kl.value, de.value, fn.value, co.value, cap.value

    def profile(self, enable=True):
        _check(self._lib.plvi_lines_profile(self._h, int(enable)), "plvi_lines_profile")

    def profile_read(self):
        ms = np.zeros(5, np.float32)
        runs = ctypes.c_int()
        _check(self._lib.plvi_lines_profile_read(self._h, _ptr(ms), ctypes.byref(runs)), "plvi_lines_profile_read")
        return dict(zip(self.STAGES, ms.tolist())), runs.value

    def kernel_timing(self, enable=True):
        """Event pair around every lsd_prep_kernel and LBD Gaussian + Sobel launch (rooflines)."""
        _check(self._lib.plvi_lines_kernel_timing(self._h, int(enable)), "plvi_lines_kernel_timing")

    def kernel_timing_read(self, kind=0):
        """(total ms, launches) since kernel_timing(True): kind 0 = lsd_prep_kernel, 1 = lbd_sobel0_kernel,
        2 = lbd_sobel1_kernel, 3 = lsd_rect_lanes_kernel (region2rect)."""
        tot = ctypes.c_float()
        n = ctypes.c_int()
        _check(self._lib.plvi_lines_kernel_timing_read_kind(self._h, int(kind), ctypes.byref(tot), ctypes.byref(n)),
               "plvi_lines_kernel_timing_read_kind")
        return tot.value, n.value

    def pyramid_level(self, level, frame=0):
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.plvi_lines_pyramid_level(self._h, frame, level, None, ctypes.byref(w), ctypes.byref(h)),
               "plvi_lines_pyramid_level")
        out = np.zeros((h.value, w.value), np.uint8)
        _check(self._lib.plvi_lines_pyramid_level(self._h, frame, level, _ptr(out), None, None),
               "plvi_lines_pyramid_level")
        return out

    def debug_planes(self, level, frame=0):
        """(deg f32, modgrad f64, cos/sin f32 [h, w, 2]) LSD planes of the last batch (diagnostic)."""
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.plvi_lines_debug_planes(self._h, frame, level, None, None, None, ctypes.byref(w),
                                                  ctypes.byref(h)), "plvi_lines_debug_planes")
        deg = np.zeros((h.value, w.value), np.float32)
        mg = np.zeros((h.value, w.value), np.float64)
        cs = np.zeros((h.value, w.value, 2), np.float32)
        _check(self._lib.plvi_lines_debug_planes(self._h, frame, level, _ptr(deg), _ptr(mg), _ptr(cs), None, None),
               "plvi_lines_debug_planes")
        return deg, mg, cs

    def debug_raw_lines(self, level, frame=0):
        """n x 4 float32 (x1, y1, x2, y2): region2rect's segments of the last batch, one per region (diagnostic)."""
        n = ctypes.c_int()
        _check(self._lib.plvi_lines_debug_raw_lines(self._h, frame, level, None, 1 << 30, ctypes.byref(n)),
               "plvi_lines_debug_raw_lines")
        out = np.zeros((max(n.value, 1), 4), np.float32)
        _check(self._lib.plvi_lines_debug_raw_lines(self._h, frame, level, _ptr(out), n.value, ctypes.byref(n)),
               "plvi_lines_debug_raw_lines")
        return out[:n.value].copy()

    def debug_sobel(self, level, frame=0):
        """(dx, dy) int16 LBD Sobel planes of the last batch (diagnostic)."""
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.plvi_lines_debug_sobel(self._h, frame, level, None, ctypes.byref(w), ctypes.byref(h)),
               "plvi_lines_debug_sobel")
        g = np.zeros((h.value, w.value, 2), np.int16)
        _check(self._lib.plvi_lines_debug_sobel(self._h, frame, level, _ptr(g), None, None), "plvi_lines_debug_sobel")
        return g[..., 0].copy(), g[..., 1].copy()

    def scale_tables(self):
        out = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        _check(self._lib.plvi_lines_scale_tables(self._h, *[_ptr(a) for a in out]), "plvi_lines_scale_tables")
        return out


def hamming_knn2(q, t):
    """BFMatcher(NORM_HAMMING).knnMatch(q, t, 2) -> (idx0, d0, idx1, d1) arrays."""
    lib = load()
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    nq, nt = q.shape[0], t.shape[0]
    out = [np.zeros(nq, np.int32) for _ in range(4)]
    _check(lib.plvi_hamming_knn2(_ptr(q), nq, _ptr(t), nt, *[_ptr(o) for o in out]), "plvi_hamming_knn2")
    return tuple(out)


def grid_csr(grid):
    """GridStructure (grid[x][y] = list of indices) -> (cols, rows, cell_off, cell_idx)."""
    cols, rows = len(grid), len(grid[0])
    off = np.zeros(cols * rows + 1, np.int32)
    idx = []
    for x in range(cols):
        for y in range(rows):
            idx.extend(grid[x][y])
            off[x * rows + y + 1] = len(idx)
    return cols, rows, off, np.array(idx if idx else [0], np.int32)


class LineMatcher:
    """ORB_SLAM3::LineMatcher static Hamming matchers (src/LineMatcher.cpp)."""

    @staticmethod
    def _inout(fn, name, desc1, desc2, nnr, matches_12):
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        prev = np.zeros(0, np.int32) if matches_12 is None else np.ascontiguousarray(matches_12, np.int32)
        m = np.full(max(d1.shape[0], prev.size, 1), -1, np.int32)
        m[:prev.size] = prev
        n = _check(fn(_ptr(d1), d1.shape[0], _ptr(d2), d2.shape[0], nnr, _ptr(m), prev.size), name)
        return n, m[:d1.shape[0]].copy()

    @staticmethod
    def matchNNR(desc1, desc2, nnr, matches_12=None):
        """LineMatcher::matchNNR (LineMatcher.cpp:41-61).  matches_12: the caller's
        existing vector (kept through resize(rows, -1) like the reference), or None."""
        lib = load()
        return LineMatcher._inout(lib.plvi_line_match_nnr_inout, "plvi_line_match_nnr_inout", desc1, desc2, nnr,
                                  matches_12)

    @staticmethod
    def match(desc1, desc2, nnr, matches_12=None):
        """LineMatcher::match(desc1, desc2, nnr, matches_12) (LineMatcher.cpp:92-111)."""
        lib = load()
        return LineMatcher._inout(lib.plvi_line_match_inout, "plvi_line_match_inout", desc1, desc2, nnr, matches_12)

    @staticmethod
    def SearchByProjection(params, cur_angle, cur_desc, grid, last_flags, last_x3dc, last_octave, ml_desc,
                           cur_blocked=None):
        """LineMatcher::SearchByProjection(CurrentFrame, LastFrame, grid, th, angth) (src/LineMatcher.cpp:274-372).
        params: LineProjParams; grid: grid[x][y] lists of current-line indices (grid_Line); last_x3dc: n x 6
        camera-frame endpoints.  Returns (count, match) with match[i2] = last-frame line index or -1."""
        lib = load()
        ca = np.ascontiguousarray(cur_angle, np.float32)
        cd = np.ascontiguousarray(cur_desc, np.uint8).reshape(-1, 32)
        cols, rows, off, idx = grid_csr(grid)
        params.grid_cols, params.grid_rows = cols, rows
        fl = np.ascontiguousarray(last_flags, np.uint8)
        x3 = np.ascontiguousarray(last_x3dc, np.float32).reshape(-1, 6)
        oc = np.ascontiguousarray(last_octave, np.int32)
        md = np.ascontiguousarray(ml_desc, np.uint8).reshape(-1, 32)
        cb = None if cur_blocked is None else np.ascontiguousarray(cur_blocked, np.uint8)
        out = np.full(max(len(ca), 1), -1, np.int32)
        n = _check(lib.plvi_line_search_projection(ctypes.byref(params), _ptr(ca), _ptr(cd),
                                                   None if cb is None else _ptr(cb), len(ca), _ptr(off), _ptr(idx),
                                                   _ptr(fl), _ptr(x3), _ptr(oc), _ptr(md), len(fl), _ptr(out)),
                   "plvi_line_search_projection")
        return n, out[:len(ca)]

    @staticmethod
    def Fuse(params, keylines, kl_desc, flags, spc, epc, dist, dot, level, ml_desc):
        """LineMatcher::Fuse(pKF, vpMapLines, th) (src/LineMatcher.cpp:373-485) as a pure search.  params:
        FuseLineParams; keylines: pKF->mvKeys_Line (KEYLINE_DTYPE) with mDescriptors_l; per MapLine (list order):
        flags (bit0 = non-NULL and not bad), spc / epc (n x 3, Rcw*SP + tcw, Rcw*EP + tcw), dist (n x 3: |0.5*(SP+EP)
        - Ow|, min / max distance invariance), dot (float64, OM.dot(pn)), level (PredictScale), descriptor.  Returns
        (nfused, fuse_idx, fuse_dist): the accepted keyline index and its distance per MapLine, else -1 / -1."""
        kl = np.ascontiguousarray(keylines).view(KEYLINE_DTYPE)
        kd = np.ascontiguousarray(kl_desc, np.uint8).reshape(-1, 32)
        fl = np.ascontiguousarray(flags, np.uint8)
        sp = np.ascontiguousarray(spc, np.float32).reshape(-1, 3)
        ep = np.ascontiguousarray(epc, np.float32).reshape(-1, 3)
        ds = np.ascontiguousarray(dist, np.float32).reshape(-1, 3)
        dt = np.ascontiguousarray(dot, np.float64)
        lv = np.ascontiguousarray(level, np.int32)
        md = np.ascontiguousarray(ml_desc, np.uint8).reshape(-1, 32)
        _same_len(len(kl), kl_desc=kd)
        _same_len(len(fl), spc=sp, epc=ep, dist=ds, dot=dt, level=lv, ml_desc=md)
        n = len(fl)
        oi = np.full(max(n, 1), -1, np.int32)
        od = np.full(max(n, 1), -1, np.int32)
        nf = _check(load().plvi_fuse_lines(ctypes.byref(params), _ptr(kl), _ptr(kd), len(kl), _ptr(fl), _ptr(sp),
                                           _ptr(ep), _ptr(ds), _ptr(dt), _ptr(lv), _ptr(md), n, _ptr(oi), _ptr(od)),
                    "plvi_fuse_lines")
        return nf, oi[:n], od[:n]

    @staticmethod
    def SearchForTriangulation(desc1, desc2, has_line1, has_line2):
        """SearchForTriangulation(pKF1, pKF2, vMatchedPairs) (src/LineMatcher.cpp:142-171): has_line =
        GetMapLine(i) != NULL per line.  Returns (nmatches, vMatchedPairs as an n x 2 int array (query, train),
        (nn_mad, nn12_mad))."""
        n1, n2 = len(desc1), len(desc2)
        c1, c2 = max(n1, 1), max(n2, 1)
        d1 = np.zeros((c1, 32), np.uint8)
        d1[:n1] = desc1
        d2 = np.zeros((c2, 32), np.uint8)
        d2[:n2] = desc2
        h1 = np.zeros(c1, np.uint8)
        h1[:n1] = has_line1
        h2 = np.zeros(c2, np.uint8)
        h2[:n2] = has_line2
        bufs = [DeviceBuffer(a.nbytes) for a in (d1, d2, h1, h2)]
        for b, a in zip(bufs, (d1, d2, h1, h2)):
            b.upload(a)
        cnt = DeviceBuffer(16)
        cnt.upload(np.array([n1, n2, 0, 0], np.int32))
        scr = DeviceBuffer(16 * c1)
        pr = DeviceBuffer(8 * c1)
        mad = DeviceBuffer(16)
        line_search_triangulation_batch(bufs[0].ptr, cnt.ptr, c1, bufs[1].ptr, cnt.ptr + 4, c2, 1, bufs[2].ptr,
                                        bufs[3].ptr, scr.ptr, pr.ptr, cnt.ptr + 8, mad.ptr)
        load().plvi_device_synchronize()
        n = int(cnt.download(np.zeros(4, np.int32))[2])
        return n, pr.download(np.zeros((c1, 2), np.int32))[:n], tuple(mad.download(np.zeros(2, np.float64)))

    @staticmethod
    def matchGrid(lines1, desc1, grid, desc2, directions2, window=((7, 0), (2, 2)), range_hint=1):
        """LineMatcher::matchGrid (src/LineMatcher.cpp:191-272).  lines1: n1 x 4 ints (line_2d grid coords),
        grid: grid[x][y] lists of right-line indices, directions2: n2 x 2.  range_hint: 1 = libstdc++ <= GCC 10
        candidate order (the reference's toolchain), 0 = GCC >= 11.  Returns (nmatches, matches_12)."""
        lib = load()
        l1 = np.ascontiguousarray(lines1, np.int32).reshape(-1, 4)
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        v2 = np.ascontiguousarray(directions2, np.float64).reshape(-1, 2)
        cols, rows, off, idx = grid_csr(grid)
        m = np.full(max(len(l1), 1), -1, np.int32)
        (w0, w1), (h0, h1) = window
        n = _check(lib.plvi_line_match_grid(_ptr(l1), _ptr(d1), len(l1), cols, rows, _ptr(off), _ptr(idx), _ptr(d2),
                                            _ptr(v2), len(d2), w0, w1, h0, h1, int(range_hint), _ptr(m)),
                   "plvi_line_match_grid")
        return n, m[:len(l1)]


def feature_vector_csr(fv):
    """DBoW2::FeatureVector (std::map<NodeId, vector<unsigned>>) as given by a
    dict {node_id: [keypoint indices]} -> (node ids ascending, offsets, indices)."""
    nodes = np.array(sorted(fv), dtype=np.int32)
    off = np.zeros(len(nodes) + 1, np.int32)
    idx = []
    for i, n in enumerate(nodes):
        idx.extend(fv[int(n)])
        off[i + 1] = len(idx)
    return nodes, off, np.array(idx, dtype=np.int32)


class ORBmatcher:
    """ORB_SLAM3::ORBmatcher(nnratio=0.6, checkOri=true) (include/ORBmatcher.h:39-68)."""

    def __init__(self, nnratio=0.6, checkOri=True):
        self._lib = load()
        self.nnratio = float(nnratio)
        self.check_orientation = bool(checkOri)

    def SearchByBoW(self, kf_desc, kf_angle, kf_live, kf_featvec, f_desc, f_angle, f_featvec, f_nleft=-1):
        """SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:269-471); f_nleft = F.Nleft
        (-1: one camera; else the two-camera branch, :321-420).  Returns (nmatches, match_kf) with
        match_kf[iF] = KF keypoint index or -1."""
        kd = np.ascontiguousarray(kf_desc, np.uint8)
        ka = np.ascontiguousarray(kf_angle, np.float32)
        kl = np.ascontiguousarray(kf_live, np.uint8)
        fd = np.ascontiguousarray(f_desc, np.uint8)
        fa = np.ascontiguousarray(f_angle, np.float32)
        kn, ko, ki = feature_vector_csr(kf_featvec)
        fn, fo, fi = feature_vector_csr(f_featvec)
        out = np.full(max(len(fd), 1), -1, np.int32)
        n = _check(self._lib.plvi_search_by_bow_stereo(self.nnratio, int(self.check_orientation), _ptr(kd),
                                                       _ptr(ka), _ptr(kl), len(kd), _ptr(kn), _ptr(ko), len(kn),
                                                       _ptr(ki), _ptr(fd), _ptr(fa), len(fd), _ptr(fn), _ptr(fo),
                                                       len(fn), _ptr(fi), int(f_nleft), _ptr(out)),
                   "plvi_search_by_bow_stereo")
        return n, out[:len(fd)]

    def SearchByBoWKF(self, desc1, angle1, live1, featvec1, desc2, angle2, live2, featvec2):
        """SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
        (src/ORBmatcher.cc:823-963), single-camera branch.  Per side: mDescriptors, mvKeysUn angles, live[i] =
        GetMapPointMatches()[i] is non-NULL and not bad, mFeatVec as {node: [indices]}.  Returns (nmatches,
        matches12) with matches12[idx1] = the KF2 keypoint index whose MapPoint goes to vpMatches12[idx1], or -1."""
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        a1 = np.ascontiguousarray(angle1, np.float32)
        a2 = np.ascontiguousarray(angle2, np.float32)
        l1 = np.ascontiguousarray(live1, np.uint8)
        l2 = np.ascontiguousarray(live2, np.uint8)
        n1, n2 = len(d1), len(d2)
        _same_len(n1, angle1=a1, live1=l1)
        _same_len(n2, angle2=a2, live2=l2)
        a, ao, ai = feature_vector_csr(featvec1)
        b, bo, bi = feature_vector_csr(featvec2)
        out = np.full(max(n1, 1), -1, np.int32)
        n = _check(self._lib.plvi_search_by_bow_kf(self.nnratio, int(self.check_orientation), _ptr(d1), _ptr(a1),
                                                   _ptr(l1), n1, _ptr(a), _ptr(ao), len(a), _ptr(ai), _ptr(d2),
                                                   _ptr(a2), _ptr(l2), n2, _ptr(b), _ptr(bo), len(b), _ptr(bi),
                                                   _ptr(out)),
                   "plvi_search_by_bow_kf")
        return n, out[:n1]

    def SearchForTriangulation(self, kps1, desc1, featvec1, has_point1, uright1, kps2, desc2, featvec2, has_point2,
                               uright2, F12, ep, sigma2, scale_factors, bOnlyStereo=False, bCoarse=False):
        """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse)
        (src/ORBmatcher.cc:965-1206), single-camera Pinhole branch.  Keypoints are mvKeysUn in
        KEYPOINT_DTYPE, has_point = GetMapPoint(i) != NULL, uright = mvuRight; F12 (3 x 3) and the epipole
        ep replace what the reference derives from the poses (plvi_frontend.h), sigma2 / scale_factors
        are pKF2's mvLevelSigma2 / mvScaleFactors.  Returns (nmatches, vMatchedPairs as an n x 2 int
        array (idx1, idx2) in idx1 order)."""
        n1, n2 = len(kps1), len(kps2)
        k1 = np.ascontiguousarray(kps1, KEYPOINT_DTYPE)
        k2 = np.ascontiguousarray(kps2, KEYPOINT_DTYPE)
        d1 = np.ascontiguousarray(desc1, np.uint8)
        d2 = np.ascontiguousarray(desc2, np.uint8)
        h1 = np.ascontiguousarray(has_point1, np.uint8)
        h2 = np.ascontiguousarray(has_point2, np.uint8)
        u1 = np.ascontiguousarray(uright1, np.float32)
        u2 = np.ascontiguousarray(uright2, np.float32)
        _same_len(n1, desc1=d1, has_point1=h1, uright1=u1)
        _same_len(n2, desc2=d2, has_point2=h2, uright2=u2)
        a, ao, ai = feature_vector_csr(featvec1)
        b, bo, bi = feature_vector_csr(featvec2)
        pair = TriangulationPair.make(F12, ep, sigma2, scale_factors, bOnlyStereo, bCoarse, self.check_orientation)
        out = np.full(max(n1, 1), -1, np.int32)
        n = _check(self._lib.plvi_search_for_triangulation(
            ctypes.byref(pair), _ptr(k1), _ptr(d1), n1, _ptr(a), _ptr(ao), len(a), _ptr(ai), _ptr(h1), _ptr(u1),
            _ptr(k2), _ptr(d2), n2, _ptr(b), _ptr(bo), len(b), _ptr(bi), _ptr(h2), _ptr(u2), _ptr(out)),
            "plvi_search_for_triangulation")
        m = out[:n1]
        i1 = np.flatnonzero(m >= 0)
        return n, np.stack([i1, m[i1]], axis=1).astype(np.int32)

    def SearchByProjection(self, params, cur_kps, cur_desc, last_x3dc, last_octave, last_angle, mp_desc,
                           last_flags, cur_blocked=None, cur_uright=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1962-2178) with
        mbCheckOrientation = checkOri of this matcher.  params: ProjParams (th, camera, grid, bounds,
        scale factors); cur_kps: mvKeysUn (KEYPOINT_DTYPE); last_*: see include/plvi_frontend.h.
        Returns (nmatches, match) with match[i2] = LastFrame index, -2 (nulled) or -1 (untouched)."""
        params.check_orientation = int(self.check_orientation)
        ck = np.ascontiguousarray(cur_kps).view(KEYPOINT_DTYPE)
        cd = np.ascontiguousarray(cur_desc, np.uint8).reshape(-1, 32)
        n = len(ck)
        x3 = np.ascontiguousarray(last_x3dc, np.float32).reshape(-1, 3)
        lo = np.ascontiguousarray(last_octave, np.int32)
        la = np.ascontiguousarray(last_angle, np.float32)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        lf = np.ascontiguousarray(last_flags, np.uint8)
        cb = None if cur_blocked is None else np.ascontiguousarray(cur_blocked, np.uint8)
        cu = None if cur_uright is None else np.ascontiguousarray(cur_uright, np.float32)
        out = np.full(max(n, 1), -1, np.int32)
        nm = _check(self._lib.plvi_search_by_projection(ctypes.byref(params), _ptr(ck), _ptr(cd), n,
                                                        None if cb is None else _ptr(cb),
                                                        None if cu is None else _ptr(cu), _ptr(x3), _ptr(lo),
                                                        _ptr(la), _ptr(md), _ptr(lf), len(lf), _ptr(out)),
                    "plvi_search_by_projection")
        return nm, out[:n]

    def SearchByProjectionLocal(self, params, kps, desc, mp_flags, mp_proj, mp_level, mp_desc, blocked=None,
                                uright=None):
        """SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
        (src/ORBmatcher.cc:44-145, monocular / rectified branch) with this matcher's nnratio.  params:
        LocalParams (grid, th, scale factors); kps: F.mvKeysUn; mp_*: per MapPoint (vector order) flags (bit0
        searched, bit1 Observations() > 0), proj (n x 4: mTrackProjX, mTrackProjY, mTrackProjXR,
        mTrackViewCos), mnTrackScaleLevel, descriptor.  Returns (nmatches, match) with match[idx] = MapPoint
        index stored in F.mvpMapPoints[idx] or -1."""
        params.nnratio = self.nnratio
        k = np.ascontiguousarray(kps).view(KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        fl = np.ascontiguousarray(mp_flags, np.uint8)
        pr = np.ascontiguousarray(mp_proj, np.float32).reshape(-1, 4)
        lv = np.ascontiguousarray(mp_level, np.int32)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        cb = None if blocked is None else np.ascontiguousarray(blocked, np.uint8)
        cu = None if uright is None else np.ascontiguousarray(uright, np.float32)
        out = np.full(max(len(k), 1), -1, np.int32)
        nm = _check(self._lib.plvi_search_local(ctypes.byref(params), _ptr(k), _ptr(d), len(k),
                                                None if cb is None else _ptr(cb), None if cu is None else _ptr(cu),
                                                _ptr(fl), _ptr(pr), _ptr(lv), _ptr(md), len(fl), _ptr(out)),
                    "plvi_search_local")
        return nm, out[:len(k)]

    def SearchByProjectionStereo(self, params, kps, desc, kps_r, desc_r, x3dc, x3dr, last_octave, last_angle,
                                 mp_desc, last_flags, kb8=None, blocked=None, blocked_r=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) with a two-camera CurrentFrame
        (CurrentFrame.Nleft != -1, src/ORBmatcher.cc:1985-2175), rotation check = checkOri of this matcher.
        params: ProjParams (camera fx/fy/cx/cy, bounds, grid, th, forward / backward, scale factors); kb8:
        KannalaBrandt8 k1..k4 (None = Pinhole); kps / desc: mvKeys and descriptor rows 0..Nleft-1; kps_r /
        desc_r: mvKeysRight and rows Nleft..; per LastFrame point: x3Dc, x3Dr = mTrl * x3Dc, octave, angle,
        descriptor, flags (bit0 MapPoint and not an outlier, bit1 Observations() > 0).  Returns (nmatches,
        match, match_r) with -2 = set to NULL by the rotation filter."""
        params.check_orientation = int(self.check_orientation)
        k = np.ascontiguousarray(kps).view(KEYPOINT_DTYPE)
        kr = np.ascontiguousarray(kps_r).view(KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        dr = np.ascontiguousarray(desc_r, np.uint8).reshape(-1, 32)
        x3 = np.ascontiguousarray(x3dc, np.float32).reshape(-1, 3)
        x3r = np.ascontiguousarray(x3dr, np.float32).reshape(-1, 3)
        lo = np.ascontiguousarray(last_octave, np.int32)
        la = np.ascontiguousarray(last_angle, np.float32)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        lf = np.ascontiguousarray(last_flags, np.uint8)
        opt = lambda a, t: None if a is None else np.ascontiguousarray(a, t)  # noqa: E731
        kb, cb, cbr = opt(kb8, np.float32), opt(blocked, np.uint8), opt(blocked_r, np.uint8)
        pp = lambda a: None if a is None else _ptr(a)  # noqa: E731
        out = np.full(max(len(k), 1), -1, np.int32)
        outr = np.full(max(len(kr), 1), -1, np.int32)
        nm = _check(self._lib.plvi_search_by_projection_stereo(
            ctypes.byref(params), pp(kb), _ptr(k), _ptr(d), len(k), pp(cb), _ptr(kr), _ptr(dr), len(kr), pp(cbr),
            _ptr(x3), _ptr(x3r), _ptr(lo), _ptr(la), _ptr(md), _ptr(lf), len(lf), _ptr(out), _ptr(outr)),
            "plvi_search_by_projection_stereo")
        return nm, out[:len(k)], outr[:len(kr)]

    def SearchByProjectionLocalStereo(self, params, kps, desc, kps_r, desc_r, mp_flags, mp_proj, mp_level,
                                      mp_proj_r, mp_level_r, mp_desc, blocked=None, blocked_r=None, l2r=None,
                                      r2l=None):
        """SearchByProjection(Frame&, const vector<MapPoint*>&, ...) on a two-camera Frame (F.Nleft != -1,
        src/ORBmatcher.cc:44-214).  kps / desc: mvKeys and descriptor rows 0..Nleft-1; kps_r / desc_r:
        mvKeysRight and rows Nleft..; blocked / blocked_r: mvpMapPoints[idx] (resp. [Nleft + idx]) with
        Observations() > 0 on entry; l2r / r2l: mvLeftToRightMatch / mvRightToLeftMatch; per MapPoint: flags
        (bit0 searched left, bit1 Observations() > 0, bit2 searched right), proj (n x 4: mTrackProjX,
        mTrackProjY, -, mTrackViewCos), mnTrackScaleLevel, proj_r (mTrackProjXR, mTrackProjYR, -,
        mTrackViewCosR), mnTrackScaleLevelR, descriptor.  Returns (nmatches, match, match_r)."""
        params.nnratio = self.nnratio
        k = np.ascontiguousarray(kps).view(KEYPOINT_DTYPE)
        kr = np.ascontiguousarray(kps_r).view(KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        dr = np.ascontiguousarray(desc_r, np.uint8).reshape(-1, 32)
        fl = np.ascontiguousarray(mp_flags, np.uint8)
        pr = np.ascontiguousarray(mp_proj, np.float32).reshape(-1, 4)
        lv = np.ascontiguousarray(mp_level, np.int32)
        prr = np.ascontiguousarray(mp_proj_r, np.float32).reshape(-1, 4)
        lvr = np.ascontiguousarray(mp_level_r, np.int32)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        opt = lambda a, t: None if a is None else np.ascontiguousarray(a, t)  # noqa: E731
        cb, cbr, a, b = opt(blocked, np.uint8), opt(blocked_r, np.uint8), opt(l2r, np.int32), opt(r2l, np.int32)
        pp = lambda a: None if a is None else _ptr(a)  # noqa: E731
        out = np.full(max(len(k), 1), -1, np.int32)
        outr = np.full(max(len(kr), 1), -1, np.int32)
        nm = _check(self._lib.plvi_search_local_stereo(ctypes.byref(params), _ptr(k), _ptr(d), len(k), pp(cb), pp(a),
                                                       _ptr(kr), _ptr(dr), len(kr), pp(cbr), pp(b), _ptr(fl), _ptr(pr),
                                                       _ptr(lv), _ptr(prr), _ptr(lvr), _ptr(md), len(fl), _ptr(out),
                                                       _ptr(outr)),
                    "plvi_search_local_stereo")
        return nm, out[:len(k)], outr[:len(kr)]

    def SearchByProjectionKF(self, params, cur_kps, cur_desc, kf_flags, x3dc, dist, level, kf_angle, mp_desc,
                             cur_blocked=None):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:2180-2300),
        the relocalization guided search, with mbCheckOrientation = checkOri of this matcher.  params:
        RelocParams (camera, bounds, grid, th, orb_dist, scale factors); cur_kps: mvKeysUn; cur_blocked:
        mvpMapPoints[i2] != NULL on entry; per KF MapPoint (GetMapPointMatches() order): flags (bit0 = live and
        not in sAlreadyFound), x3dc (n x 3), dist (n x 3: dist3D, min / max distance invariance), level
        (PredictScale), kf_angle (pKF->mvKeysUn[i].angle), descriptor.  Returns (nmatches, match) with
        match[i2] = KF MapPoint index, -2 (nulled by the rotation filter) or -1 (untouched)."""
        params.check_orientation = int(self.check_orientation)
        ck = np.ascontiguousarray(cur_kps).view(KEYPOINT_DTYPE)
        cd = np.ascontiguousarray(cur_desc, np.uint8).reshape(-1, 32)
        n = len(ck)
        fl = np.ascontiguousarray(kf_flags, np.uint8)
        x3 = np.ascontiguousarray(x3dc, np.float32).reshape(-1, 3)
        ds = np.ascontiguousarray(dist, np.float32).reshape(-1, 3)
        lv = np.ascontiguousarray(level, np.int32)
        ka = np.ascontiguousarray(kf_angle, np.float32)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        cb = None if cur_blocked is None else np.ascontiguousarray(cur_blocked, np.uint8)
        out = np.full(max(n, 1), -1, np.int32)
        nm = _check(self._lib.plvi_search_reloc(ctypes.byref(params), _ptr(ck), _ptr(cd), n,
                                                None if cb is None else _ptr(cb), _ptr(fl), _ptr(x3), _ptr(ds),
                                                _ptr(lv), _ptr(ka), _ptr(md), len(fl), _ptr(out)),
                    "plvi_search_reloc")
        return nm, out[:n]

    def SearchByProjectionSim3(self, params, kps, desc, flags, x3dc, dist, dot, level, mp_desc, matched=None,
                               projection=0):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (src/ORBmatcher.cc:473-586,
        projection=0) and the overload with vpPointsKFs / vpMatchedKF (:588-704, projection=1), the loop-closing
        guided searches.  params: Sim3ProjParams (camera, bounds, grid, th, ratio_hamming, scale factors; its
        projection field is set from the argument); kps: pKF->mvKeysUn; matched: vpMatched[idx] != NULL on entry;
        per candidate MapPoint (vpPoints order): flags (bit0 = not bad and not in spAlreadyFound), x3dc (n x 3,
        Rcw*p3Dw + tcw), dist (n x 3: |p3Dw - Ow|, min / max distance invariance), dot (float64, PO.dot(Pn)), level
        (PredictScale), descriptor.  Returns (nmatches, match) with match[idx] = the point index stored in
        vpMatched[idx] by this call, or -1; vpMatchedKF[idx] is vpPointsKFs[match[idx]]."""
        params.projection = int(projection)
        k = np.ascontiguousarray(kps).view(KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(k)
        fl = np.ascontiguousarray(flags, np.uint8)
        x3 = np.ascontiguousarray(x3dc, np.float32).reshape(-1, 3)
        ds = np.ascontiguousarray(dist, np.float32).reshape(-1, 3)
        dt = np.ascontiguousarray(dot, np.float64)
        lv = np.ascontiguousarray(level, np.int32)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        _same_len(n, desc=d)
        _same_len(len(fl), x3dc=x3, dist=ds, dot=dt, level=lv, mp_desc=md)
        mb = None if matched is None else np.ascontiguousarray(matched, np.uint8)
        out = np.full(max(n, 1), -1, np.int32)
        nm = _check(self._lib.plvi_search_sim3_projection(ctypes.byref(params), _ptr(k), _ptr(d), n,
                                                          None if mb is None else _ptr(mb), _ptr(fl), _ptr(x3),
                                                          _ptr(ds), _ptr(dt), _ptr(lv), _ptr(md), len(fl), _ptr(out)),
                    "plvi_search_sim3_projection")
        return nm, out[:n]

    def _fuse(self, mode, params, kps, desc, flags, x3dc, dist, dot, level, mp_desc, uright):
        params.mode = mode
        k = np.ascontiguousarray(kps).view(KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        fl = np.ascontiguousarray(flags, np.uint8)
        x3 = np.ascontiguousarray(x3dc, np.float32).reshape(-1, 3)
        ds = np.ascontiguousarray(dist, np.float32).reshape(-1, 3)
        dt = np.ascontiguousarray(dot, np.float64)
        lv = np.ascontiguousarray(level, np.int32)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
        _same_len(len(k), desc=d, **({} if ur is None else {"uright": ur}))
        _same_len(len(fl), x3dc=x3, dist=ds, dot=dt, level=lv, mp_desc=md)
        n = len(fl)
        oi = np.full(max(n, 1), -1, np.int32)
        od = np.full(max(n, 1), -1, np.int32)
        nf = _check(self._lib.plvi_fuse_points(ctypes.byref(params), _ptr(k), _ptr(d), len(k),
                                               None if ur is None else _ptr(ur), _ptr(fl), _ptr(x3), _ptr(ds),
                                               _ptr(dt), _ptr(lv), _ptr(md), n, _ptr(oi), _ptr(od)),
                    "plvi_fuse_points")
        return nf, oi[:n], od[:n]

    def Fuse(self, params, kps, desc, flags, x3dc, dist, dot, level, mp_desc, uright=None):
        """Fuse(pKF, vpMapPoints, th, bRight=false) (src/ORBmatcher.cc:1399-1610) as a pure search.  params:
        FuseParams (camera, bounds, grid, th, bf, scale factors, mvInvLevelSigma2; its mode field is set here); kps:
        pKF->mvKeysUn with mDescriptors; uright: pKF->mvuRight (None = monocular); per candidate MapPoint (list
        order): flags (bit0 = non-NULL, not bad and not in pKF on entry), x3dc (n x 3, Rcw*p3Dw + tcw), dist (n x 3:
        |p3Dw - Ow|, min / max distance invariance), dot (float64, PO.dot(Pn)), level (PredictScale), descriptor.
        Returns (nfused, fuse_idx, fuse_dist): per point the accepted keypoint index (bestIdx) and its distance,
        else -1 / -1; the caller replays the map mutation in list order."""
        return self._fuse(0, params, kps, desc, flags, x3dc, dist, dot, level, mp_desc, uright)

    def FuseSim3(self, params, kps, desc, flags, x3dc, dist, dot, level, mp_desc):
        """Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1612-1734) as a pure search: no
        reprojection gate; flags bit0 = not bad and not in spAlreadyFound; x3dc from the decomposed Scw.  Returns as
        Fuse; vpReplacePoint[i] is pKF->GetMapPoint(fuse_idx[i]) on the caller's side."""
        return self._fuse(1, params, kps, desc, flags, x3dc, dist, dot, level, mp_desc, None)

    @staticmethod
    def DescriptorDistance(a, b, line_matcher_quirk=False):
        """Row-wise distances of two n x 32 descriptor tables on the GPU."""
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        n = a.shape[0]
        lib = load()
        da, db, do = DeviceBuffer(max(a.nbytes, 32)), DeviceBuffer(max(b.nbytes, 32)), DeviceBuffer(max(4 * n, 4))
        da.upload(a)
        db.upload(b)
        _check(lib.plvi_descriptor_distance_batch(ctypes.c_void_p(da.ptr), ctypes.c_void_p(db.ptr), n,
                                                  int(line_matcher_quirk), ctypes.c_void_p(do.ptr), None),
               "plvi_descriptor_distance_batch")
        lib.plvi_device_synchronize()
        return do.download(np.zeros(n, np.int32))


def frame_extract_batch(orb, lines, d_frames_ptr, n_frames, frame_stride, row_stride, lap=(0, 0), stream=None):
    """Frame::Frame's ORB + line extraction of a device batch as one schedule
    (plvi_frame_extract_batch); results via orb.outputs() / lines.outputs()."""
    _check(load().plvi_frame_extract_batch(orb._h, lines._h, ctypes.c_void_p(d_frames_ptr), n_frames, frame_stride,
                                           row_stride, lap[0], lap[1], ctypes.c_void_p(stream or 0)),
           "plvi_frame_extract_batch")


def frame_extract_match_batch(orb, lines, d_frames_ptr, n_frames, frame_stride, row_stride, knn_out, nnr,
                              line_scratch, line_matches, line_nmatch, lap=(0, 0), stream=None):
    """plvi_frame_extract_match_batch: the frame schedule plus the step's matching of frame t vs t-1 (ORB
    kNN-2 into knn_out = (idx0, d0, idx1, d1) device pointers, LineMatcher::match into line_matches /
    line_nmatch) issued inside the schedule's streams."""
    V = ctypes.c_void_p
    _check(load().plvi_frame_extract_match_batch(orb._h, lines._h, V(d_frames_ptr), n_frames, frame_stride, row_stride,
                                                 lap[0], lap[1], *[V(p) for p in knn_out], ctypes.c_float(nnr),
                                                 V(line_scratch), V(line_matches), V(line_nmatch), V(stream or 0)),
           "plvi_frame_extract_match_batch")


def frame_orb_event(lines):
    """plvi_frame_orb_event: the hipEvent_t the last frame_extract_batch on `lines` recorded when its ORB
    part completed (handle-owned)."""
    e = ctypes.c_void_p()
    _check(load().plvi_frame_orb_event(lines._h, ctypes.byref(e)), "plvi_frame_orb_event")
    return e.value


def event_create():
    e = ctypes.c_void_p()
    _check(load().plvi_event_create(ctypes.byref(e)), "plvi_event_create")
    return e.value


def event_record(event, stream=None):
    _check(load().plvi_event_record(ctypes.c_void_p(event), ctypes.c_void_p(stream or 0)), "plvi_event_record")


def stream_wait_event(stream, event):
    _check(load().plvi_stream_wait_event(ctypes.c_void_p(stream or 0), ctypes.c_void_p(event)),
           "plvi_stream_wait_event")


def event_destroy(event):
    _check(load().plvi_event_destroy(ctypes.c_void_p(event)), "plvi_event_destroy")


def stereo_frame_extract_batch(orb_left, orb_right, lines_left, lines_right, d_left_ptr, d_right_ptr, n_frames,
                               frame_stride, row_stride, lap=(0, 0), stream=None):
    """The stereo-line Frame's four extractions (plvi_stereo_frame_extract_batch)."""
    V = ctypes.c_void_p
    _check(load().plvi_stereo_frame_extract_batch(orb_left._h, orb_right._h, lines_left._h, lines_right._h,
                                                  V(d_left_ptr), V(d_right_ptr), n_frames, frame_stride, row_stride,
                                                  lap[0], lap[1], V(stream or 0)), "plvi_stereo_frame_extract_batch")


class StepGraph:
    """A batch step captured into a HIP graph (plvi_graph_*): ``fn(stream)``
    issues plvi_* calls on ``stream`` (a created stream); the graph replays
    them with one launch.  The captured pointers and parameters are fixed."""

    def __init__(self, fn, stream):
        self._lib = load()
        self._stream = stream
        _check(self._lib.plvi_graph_capture_begin(ctypes.c_void_p(stream)), "plvi_graph_capture_begin")
        try:
            fn(stream)
        finally:
            ex = ctypes.c_void_p()
            rc = self._lib.plvi_graph_capture_end(ctypes.c_void_p(stream), ctypes.byref(ex))
        _check(rc, "plvi_graph_capture_end")
        self._exec = ex

    def launch(self, stream=None):
        _check(self._lib.plvi_graph_launch(self._exec, ctypes.c_void_p(stream or self._stream)), "plvi_graph_launch")

    def __del__(self):
        if getattr(self, "_exec", None):
            self._lib.plvi_graph_destroy(self._exec)
            self._exec = None


class ORBVocabulary:
    """DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (ORBVocabulary.h) on the GPU.

    ``ORBVocabulary.loadFromTextFile(path)`` mirrors the reference loader
    (TemplatedVocabulary.h:1338-1424); ``ORBVocabulary.from_nodes(...)`` builds
    the same structure from a node table.  ``transform(desc, levelsup)``
    returns ``(BowVector, FeatureVector)`` as dicts {word: value} and
    {node: [feature indices]} in std::map (ascending key) order
    (TemplatedVocabulary.h:1126-1194).
    """

    def __init__(self, handle):
        self._lib = load()
        self._h = handle
        info = np.zeros(6, np.int32)
        _check(self._lib.plvi_vocab_info(self._h, _ptr(info)), "plvi_vocab_info")
        self.k, self.L, self.scoring, self.weighting, self.n_nodes, self.n_words = (int(x) for x in info)

    @classmethod
    def loadFromTextFile(cls, path, emulate_tail=False, device=0):
        """TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1424).  emulate_tail=True adds
        the node the reference's `while(!f.eof()) getline` loop reads from the empty tail after a final
        newline -- undefined in the reference (pid / nIsLeaf / the descriptor stay unassigned), modelled here
        as a zero-descriptor non-word child of the root; off by default."""
        h = ctypes.c_void_p()
        _check(load().plvi_vocab_load_text(str(path).encode(), int(emulate_tail), device, ctypes.byref(h)),
               "plvi_vocab_load_text")
        return cls(h)

    @classmethod
    def from_nodes(cls, k, L, scoring, weighting, parent, is_leaf, desc, weight, device=0):
        parent = np.ascontiguousarray(parent, np.int32)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, np.float64)
        h = ctypes.c_void_p()
        _check(load().plvi_vocab_create(k, L, scoring, weighting, len(parent), _ptr(parent), _ptr(is_leaf),
                                        _ptr(desc), _ptr(weight), device, ctypes.byref(h)), "plvi_vocab_create")
        return cls(h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.plvi_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def empty(self):
        return self.n_words == 0

    def transform_arrays(self, desc, levelsup=4):
        """Raw CSR form: (bow_word, bow_value, fv_node, fv_off, fv_idx)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = d.shape[0]
        m = max(n, 1)
        bw, bv = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fn, fo, fi = np.zeros(m, np.uint32), np.zeros(m + 1, np.int32), np.zeros(m, np.uint32)
        nb, nf = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.plvi_vocab_transform(self._h, _ptr(d), n, levelsup, _ptr(bw), _ptr(bv), ctypes.byref(nb),
                                              _ptr(fn), _ptr(fo), _ptr(fi), ctypes.byref(nf)), "plvi_vocab_transform")
        nb, nf = nb.value, nf.value
        return bw[:nb], bv[:nb], fn[:nf], fo[:nf + 1], fi[:fo[nf]]

    def transform(self, desc, levelsup=4):
        bw, bv, fn, fo, fi = self.transform_arrays(desc, levelsup)
        bow = {int(w): float(v) for w, v in zip(bw, bv)}
        fv = {int(fn[i]): [int(x) for x in fi[fo[i]:fo[i + 1]]] for i in range(len(fn))}
        return bow, fv

    def transform_features(self, desc, levelsup=4):
        """Per-descriptor (word ids, node ids at level L - levelsup)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = d.shape[0]
        w, ni = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        _check(self._lib.plvi_vocab_transform_features(self._h, _ptr(d), n, levelsup, _ptr(w), _ptr(ni)),
               "plvi_vocab_transform_features")
        return w[:n], ni[:n]


def _bow_arrays(bow):
    """A BowVector as (ascending uint32 words, float64 values): a {word: value} dict or a (words, values) pair."""
    if isinstance(bow, dict):
        ws = sorted(bow)
        return np.array(ws, np.uint32), np.array([bow[w] for w in ws], np.float64)
    w, v = bow
    return np.ascontiguousarray(w, np.uint32), np.ascontiguousarray(v, np.float64)


def pack_bow(bows, cap=None):
    """BowVectors -> the [frame][cap] tables of plvi_vocab_transform_batch: (word, value, n)."""
    arrs = [_bow_arrays(b) for b in bows]
    cap = max([len(w) for w, _ in arrs] + [1]) if cap is None else cap
    word, value = np.zeros((len(arrs), cap), np.uint32), np.zeros((len(arrs), cap), np.float64)
    n = np.zeros(max(len(arrs), 1), np.int32)
    for i, (w, v) in enumerate(arrs):
        word[i, :len(w)], value[i, :len(w)], n[i] = w, v, len(w)
    return word, value, n


def kfdb_add_batch(db, entries, d_bow_word, d_bow_value, d_bow_n, cap, stream=None):
    """KeyFrameDatabase::add of device BowVector tables (plvi_kfdb_add_batch).  entries: host n x 3 ints
    (frame row, slot, map id).  Asynchronous on `stream`."""
    V = ctypes.c_void_p
    e = np.ascontiguousarray(entries, np.int32).reshape(-1, 3)
    _check(load().plvi_kfdb_add_batch(db._h, len(e), _ptr(e), V(d_bow_word or 0), V(d_bow_value or 0), V(d_bow_n), cap,
                                      V(stream or 0)), "plvi_kfdb_add_batch")


def kfdb_query_batch(db, n_queries, d_q_word, d_q_value, d_q_n, q_cap, d_q_map, mode, n_best=3, d_conn_off=0,
                     d_conn_slot=0, d_covis=0, d_map_bad=0, n_maps=0, d_words=0, d_score=0, d_order=0, d_norder=0,
                     d_cand=0, cand_cap=0, d_ncand=0, d_loop=0, d_nloop=0, d_merge=0, d_nmerge=0, stream=None):
    """DetectRelocalizationCandidates (mode 0) / DetectNBestCandidates (mode 1) of n_queries device BowVectors
    (plvi_kfdb_query_batch; every pointer is a device address, 0 = NULL).  Asynchronous on `stream`."""
    V = ctypes.c_void_p
    _check(load().plvi_kfdb_query_batch(db._h, n_queries, V(d_q_word or 0), V(d_q_value or 0), V(d_q_n), q_cap,
                                        V(d_q_map), mode, n_best, V(d_conn_off or 0), V(d_conn_slot or 0),
                                        V(d_covis or 0), V(d_map_bad or 0), n_maps, V(d_words or 0), V(d_score or 0),
                                        V(d_order or 0), V(d_norder or 0), V(d_cand or 0), cand_cap, V(d_ncand or 0),
                                        V(d_loop or 0), V(d_nloop or 0), V(d_merge or 0), V(d_nmerge or 0),
                                        V(stream or 0)), "plvi_kfdb_query_batch")


class KeyFrameDatabase:
    """ORB_SLAM3::KeyFrameDatabase (src/KeyFrameDatabase.cc) on the GPU: keyframes live in caller-chosen slots
    [0, slot_cap) and every method speaks slot numbers.  ``voc`` is an ORBVocabulary (its word count and scoring
    type are taken; only L1_NORM is supported) or a word count.  BowVectors are {word: value} dicts or
    (words, values) pairs."""

    def __init__(self, voc, slot_cap, word_cap, scoring=0, device=0):
        self._lib = load()
        n_words = voc.n_words if hasattr(voc, "n_words") else int(voc)
        scoring = voc.scoring if hasattr(voc, "scoring") else scoring
        h = ctypes.c_void_p()
        _check(self._lib.plvi_kfdb_create(n_words, slot_cap, word_cap, scoring, device, ctypes.byref(h)),
               "plvi_kfdb_create")
        self._h, self.n_words, self.slot_cap, self.word_cap = h, n_words, slot_cap, word_cap

    def close(self):
        if getattr(self, "_h", None):
            self._lib.plvi_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, slot, bow, map_id=0):
        w, v = _bow_arrays(bow)
        _check(self._lib.plvi_kfdb_add(self._h, slot, map_id, _ptr(w), _ptr(v), len(w)), "plvi_kfdb_add")

    def add_many(self, slots, bows, map_ids):
        """add of several keyframes in the given order through plvi_kfdb_add_batch."""
        word, value, n = pack_bow(bows)
        bufs = [DeviceBuffer(a.nbytes) for a in (word, value, n)]
        for b, a in zip(bufs, (word, value, n)):
            b.upload(a)
        entries = np.stack([np.arange(len(slots)), np.asarray(slots), np.asarray(map_ids)], axis=1)
        kfdb_add_batch(self, entries, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, word.shape[1])
        return self.errors()

    def erase(self, slots, stream=None):
        s = np.atleast_1d(np.asarray(slots, np.int32))
        _check(self._lib.plvi_kfdb_erase(self._h, len(s), _ptr(s), ctypes.c_void_p(stream or 0)), "plvi_kfdb_erase")

    def clearMap(self, map_id, stream=None):
        _check(self._lib.plvi_kfdb_clear_map(self._h, map_id, ctypes.c_void_p(stream or 0)), "plvi_kfdb_clear_map")

    def clear(self, stream=None):
        _check(self._lib.plvi_kfdb_clear(self._h, ctypes.c_void_p(stream or 0)), "plvi_kfdb_clear")

    def errors(self, stream=None):
        """Read and clear the error word (bit 0: a count above word_cap, bit 1: a word id >= n_words)."""
        f = ctypes.c_int()
        self._lib.plvi_kfdb_errors(self._h, ctypes.byref(f), ctypes.c_void_p(stream or 0))
        return f.value

    def _covis(self, covis):
        if covis is None:
            return None
        c = np.ascontiguousarray(covis, np.int32)
        if c.shape != (self.slot_cap, KFDB_NEIGHBOURS):
            raise ValueError("covis: slot_cap x 10 slots, -1 ends a row")
        return c

    def DetectRelocalizationCandidates(self, bow, map_id, covis=None, cand_cap=None):
        """vpRelocCandidates as slots, in the reference's order (KeyFrameDatabase.cc:790-902)."""
        w, v = _bow_arrays(bow)
        c = self._covis(covis)
        cap = self.slot_cap if cand_cap is None else cand_cap
        cand = np.full(max(cap, 1), -1, np.int32)
        n = _check(self._lib.plvi_kfdb_query(self._h, _ptr(w), _ptr(v), len(w), map_id, 0, 0, None, 0,
                                             None if c is None else _ptr(c), None, 0, _ptr(cand), cap, None, None,
                                             None, None), "plvi_kfdb_query")
        return [int(x) for x in cand[:min(n, cap)]]

    def DetectNBestCandidates(self, bow, map_id, connected=(), n_best=3, covis=None, map_bad=None):
        """(vpLoopCand, vpMergeCand) as slots (KeyFrameDatabase.cc:619-787)."""
        w, v = _bow_arrays(bow)
        c = self._covis(covis)
        conn = np.ascontiguousarray(sorted(connected), np.int32)
        bad = None if map_bad is None else np.ascontiguousarray(map_bad, np.uint8)
        loop, merge = np.full(max(n_best, 1), -1, np.int32), np.full(max(n_best, 1), -1, np.int32)
        nl, nm = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.plvi_kfdb_query(self._h, _ptr(w), _ptr(v), len(w), map_id, 1, n_best,
                                         _ptr(conn) if len(conn) else None, len(conn),
                                         None if c is None else _ptr(c), None if bad is None else _ptr(bad),
                                         0 if bad is None else len(bad), None, 0, _ptr(loop), ctypes.byref(nl),
                                         _ptr(merge), ctypes.byref(nm)), "plvi_kfdb_query")
        return [int(x) for x in loop[:nl.value]], [int(x) for x in merge[:nm.value]]

    def query_arrays(self, bows, map_ids, mode, n_best=3, connected=None, covis=None, map_bad=None, cand_cap=None,
                     q_cap=None, counts=None, fill=-7):
        """One plvi_kfdb_query_batch call from host data with every stage output downloaded: a dict of words, score,
        order, norder and cand / ncand (mode 0) or loop / nloop / merge / nmerge (mode 1).  Outputs are pre-filled
        with `fill` (score with NaN) so that unwritten cells show.  `counts` overrides the per-query counts (to
        pass values outside [0, q_cap])."""
        nq, S = len(bows), self.slot_cap
        word, value, n = pack_bow(bows, q_cap)
        if counts is not None:
            n = np.ascontiguousarray(counts, np.int32)
        c = self._covis(covis)
        conn = [sorted(x) for x in connected] if connected is not None else None
        ins = {"word": word, "value": value, "n": n, "map": np.ascontiguousarray(map_ids, np.int32)}
        if conn is not None:
            off = np.zeros(nq + 1, np.int32)
            off[1:] = np.cumsum([len(x) for x in conn])
            ins["coff"], ins["cslot"] = off, np.array([s for x in conn for s in x] + [0], np.int32)
        if c is not None:
            ins["covis"] = c
        if map_bad is not None:
            ins["bad"] = np.ascontiguousarray(map_bad, np.uint8)
        cap = S if cand_cap is None else cand_cap
        outs = {"words": np.full((nq, S), fill, np.int32), "score": np.full((nq, S), np.nan, np.float64),
                "order": np.full((nq, S), fill, np.int32), "norder": np.full(nq, fill, np.int32)}
        if mode == 0:
            outs.update(cand=np.full((nq, max(cap, 1)), fill, np.int32), ncand=np.full(nq, fill, np.int32))
        else:
            outs.update(loop=np.full((nq, max(n_best, 1)), fill, np.int32), nloop=np.full(nq, fill, np.int32),
                        merge=np.full((nq, max(n_best, 1)), fill, np.int32), nmerge=np.full(nq, fill, np.int32))
        d = {}
        for k, a in list(ins.items()) + list(outs.items()):
            d[k] = DeviceBuffer(a.nbytes)
            d[k].upload(a)
        g = lambda k: d[k].ptr if k in d else 0  # noqa: E731
        kfdb_query_batch(self, nq, g("word"), g("value"), g("n"), word.shape[1], g("map"), mode, n_best, g("coff"),
                         g("cslot"), g("covis"), g("bad"), len(ins["bad"]) if "bad" in ins else 0, g("words"),
                         g("score"), g("order"), g("norder"), g("cand"), cap, g("ncand"), g("loop"), g("nloop"),
                         g("merge"), g("nmerge"))
        _check(self._lib.plvi_device_synchronize(), "plvi_device_synchronize")
        for k, a in outs.items():
            d[k].download(a)
        return outs


def assign_grid_batch(d_kps, d_count, cap, n_frames, grid, d_cell_off, d_cell_idx, stream=None):
    """Frame::AssignFeaturesToGrid (src/Frame.cc:644-675) of device keypoint tables -> CSR grids."""
    _check(load().plvi_assign_grid_batch(ctypes.c_void_p(d_kps), ctypes.c_void_p(d_count), cap, n_frames,
                                         ctypes.byref(grid), ctypes.c_void_p(d_cell_off),
                                         ctypes.c_void_p(d_cell_idx), ctypes.c_void_p(stream or 0)),
           "plvi_assign_grid_batch")


# ------------------------------------------------------- initialization
def search_for_initialization_batch(n_pairs, params, d_kps1, d_desc1, d_n1, cap1, d_prev, d_kps2, d_desc2, d_n2, cap2,
                                    d_cell_off, d_cell_idx, d_m12, d_nm, stream=None):
    """ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:705-814) over device pair tables."""
    V = ctypes.c_void_p
    _check(load().plvi_search_for_initialization_batch(n_pairs, ctypes.byref(params), V(d_kps1), V(d_desc1), V(d_n1),
                                                       cap1, V(d_prev), V(d_kps2), V(d_desc2), V(d_n2), cap2,
                                                       V(d_cell_off), V(d_cell_idx), V(d_m12), V(d_nm),
                                                       V(stream or 0)),
           "plvi_search_for_initialization_batch")


def search_for_initialization(kps1, desc1, prev_xy, kps2, desc2, width=640, height=480, window=100, nnratio=0.9,
                              check_orientation=True, grid=None):
    """One (F1, F2) pair from host arrays (keypoints in KEYPOINT_DTYPE = mvKeysUn,
    descriptors n x 32, prev_xy = vbPrevMatched n1 x 2): returns (nmatches,
    vnMatches12, updated vbPrevMatched).  grid = (min_x, min_y, inv_w, inv_h)
    (default: the Frame grid of an undistorted width x height image)."""
    n1, n2 = len(kps1), len(kps2)
    if grid is None:
        g = grid_geometry(width, height)
        grid = (g[0], g[2], g[4], g[5])
    p = InitParams(float(grid[0]), float(grid[1]), float(grid[2]), float(grid[3]), int(window), float(nnratio),
                   int(bool(check_orientation)))
    c1, c2 = max(n1, 1), max(n2, 1)
    k1 = np.zeros(c1, KEYPOINT_DTYPE)
    k1[:n1] = kps1
    k2 = np.zeros(c2, KEYPOINT_DTYPE)
    k2[:n2] = kps2
    d1 = np.zeros((c1, 32), np.uint8)
    d1[:n1] = desc1
    d2 = np.zeros((c2, 32), np.uint8)
    d2[:n2] = desc2
    pv = np.zeros((c1, 2), np.float32)
    pv[:n1] = prev_xy
    bufs = [DeviceBuffer(a.nbytes) for a in (k1, d1, pv, k2, d2)]
    for b, a in zip(bufs, (k1, d1, pv, k2, d2)):
        b.upload(a)
    cnt = DeviceBuffer(16)
    cnt.upload(np.array([n1, n2, 0, 0], np.int32))
    co = DeviceBuffer(4 * 3073)
    ci = DeviceBuffer(4 * c2)
    m = DeviceBuffer(4 * c1)
    assign_grid_batch(bufs[3].ptr, cnt.ptr + 4, c2, 1, GridParams(*[float(v) for v in grid]), co.ptr, ci.ptr)
    search_for_initialization_batch(1, p, bufs[0].ptr, bufs[1].ptr, cnt.ptr, c1, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr,
                                    cnt.ptr + 4, c2, co.ptr, ci.ptr, m.ptr, cnt.ptr + 8)
    load().plvi_device_synchronize()
    out = cnt.download(np.zeros(4, np.int32))
    return int(out[2]), m.download(np.zeros(c1, np.int32))[:n1], bufs[2].download(np.zeros((c1, 2), np.float32))[:n1]


def line_search_init_batch(d_desc1, d_n1, cap1, d_desc2, d_n2, cap2, n_pairs, d_scratch, d_pairs, d_npairs, d_mad=0,
                           stream=None):
    """LineMatcher::SerachForInitialize + Frame::lineDescriptorMAD over device pair tables."""
    V = ctypes.c_void_p
    _check(load().plvi_line_search_init_batch(V(d_desc1), V(d_n1), cap1, V(d_desc2), V(d_n2), cap2, n_pairs,
                                              V(d_scratch), V(d_pairs), V(d_npairs), V(d_mad), V(stream or 0)),
           "plvi_line_search_init_batch")


def line_search_triangulation_batch(d_desc1, d_n1, cap1, d_desc2, d_n2, cap2, n_pairs, d_has_line1, d_has_line2,
                                    d_scratch, d_pairs, d_npairs, d_mad=0, stream=None):
    """LineMatcher::SearchForTriangulation (src/LineMatcher.cpp:142-171) over device pair tables."""
    V = ctypes.c_void_p
    _check(load().plvi_line_search_triangulation_batch(V(d_desc1), V(d_n1), cap1, V(d_desc2), V(d_n2), cap2, n_pairs,
                                                       V(d_has_line1), V(d_has_line2), V(d_scratch), V(d_pairs),
                                                       V(d_npairs), V(d_mad), V(stream or 0)),
           "plvi_line_search_triangulation_batch")


def search_for_triangulation_batch(n_pairs, d_pairs, cap1, cap2, node_cap, kf1, kf2, d_matches12, d_nmatches,
                                   stream=None):
    """ORBmatcher::SearchForTriangulation over device pair tables (plvi_search_for_triangulation_batch).
    d_pairs: TriangulationPair [n_pairs]; kf1 / kf2: the nine device pointers of one side in header order
    (kps, desc, n, node, off, nnodes, idx, has_point, uright)."""
    V = ctypes.c_void_p
    if len(kf1) != 9 or len(kf2) != 9:
        raise ValueError("kf1 / kf2: nine device pointers each")
    _check(load().plvi_search_for_triangulation_batch(n_pairs, V(d_pairs), cap1, cap2, node_cap,
                                                      *[V(x) for x in kf1], *[V(x) for x in kf2], V(d_matches12),
                                                      V(d_nmatches), V(stream or 0)),
           "plvi_search_for_triangulation_batch")


def search_by_bow_kf_batch(n_pairs, nnratio, check_orientation, cap1, cap2, node_cap, kf1, kf2, d_matches12,
                           d_nmatches, stream=None):
    """ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*) over device pair tables (plvi_search_by_bow_kf_batch).
    kf1 / kf2: the eight device pointers of one side in header order (desc, angle, live, n, node, off, nnodes,
    idx)."""
    V = ctypes.c_void_p
    if len(kf1) != 8 or len(kf2) != 8:
        raise ValueError("kf1 / kf2: eight device pointers each")
    _check(load().plvi_search_by_bow_kf_batch(n_pairs, float(nnratio), int(check_orientation), cap1, cap2, node_cap,
                                              *[V(x) for x in kf1], *[V(x) for x in kf2], V(d_matches12),
                                              V(d_nmatches), V(stream or 0)),
           "plvi_search_by_bow_kf_batch")


def search_sim3_projection_batch(n_pairs, params, kf, kp_cap, points, pt_cap, d_match, d_nmatches, stream=None):
    """Both ORBmatcher::SearchByProjection(pKF, Scw, ...) overloads over device tables
    (plvi_search_sim3_projection_batch).  params: Sim3ProjParams; kf: the six device pointers of the keyframe
    side in header order (kps, desc, n, matched (0 = none), cell_off, cell_idx); points: the seven of the point
    side (flags, x3dc, dist, dot, level, desc, n)."""
    V = ctypes.c_void_p
    if len(kf) != 6 or len(points) != 7:
        raise ValueError("kf: six device pointers, points: seven")
    kps, desc, n, matched, cell_off, cell_idx = kf
    flags, x3dc, dist, dot, level, mp_desc, pt_n = points
    _check(load().plvi_search_sim3_projection_batch(n_pairs, ctypes.byref(params), V(kps), V(desc), V(n), kp_cap,
                                                    V(matched or 0), V(cell_off), V(cell_idx), V(flags), V(x3dc),
                                                    V(dist), V(dot), V(level), V(mp_desc), V(pt_n), pt_cap,
                                                    V(d_match), V(d_nmatches), V(stream or 0)),
           "plvi_search_sim3_projection_batch")


def fuse_points_batch(n_pairs, params, kf, kp_cap, points, pt_cap, d_fuse_idx, d_fuse_dist, d_nfused, stream=None):
    """Both ORBmatcher::Fuse overloads over device tables (plvi_fuse_points_batch).  params: FuseParams (mode set by
    the caller); kf: the six device pointers of the keyframe side in header order (kps, desc, n, uright (0 =
    monocular), cell_off, cell_idx); points: the seven of the point side (flags, x3dc, dist, dot, level, desc, n).
    nfused is written by the call."""
    V = ctypes.c_void_p
    if len(kf) != 6 or len(points) != 7:
        raise ValueError("kf: six device pointers, points: seven")
    kps, desc, n, uright, cell_off, cell_idx = kf
    flags, x3dc, dist, dot, level, mp_desc, pt_n = points
    _check(load().plvi_fuse_points_batch(n_pairs, ctypes.byref(params), V(kps), V(desc), V(n), kp_cap,
                                         V(uright or 0), V(cell_off), V(cell_idx), V(flags), V(x3dc), V(dist),
                                         V(dot), V(level), V(mp_desc), V(pt_n), pt_cap, V(d_fuse_idx),
                                         V(d_fuse_dist), V(d_nfused), V(stream or 0)),
           "plvi_fuse_points_batch")


def fuse_lines_batch(n_pairs, params, kf, kl_cap, lines, ml_cap, d_fuse_idx, d_fuse_dist, d_nfused, stream=None):
    """LineMatcher::Fuse over device tables (plvi_fuse_lines_batch).  params: FuseLineParams; kf: the three device
    pointers of the keyframe side (keylines, desc, n); lines: the eight of the MapLine side (flags, spc, epc, dist,
    dot, level, desc, n)."""
    V = ctypes.c_void_p
    if len(kf) != 3 or len(lines) != 8:
        raise ValueError("kf: three device pointers, lines: eight")
    kl, kl_desc, kl_n = kf
    flags, spc, epc, dist, dot, level, ml_desc, ml_n = lines
    _check(load().plvi_fuse_lines_batch(n_pairs, ctypes.byref(params), V(kl), V(kl_desc), V(kl_n), kl_cap, V(flags),
                                        V(spc), V(epc), V(dist), V(dot), V(level), V(ml_desc), V(ml_n), ml_cap,
                                        V(d_fuse_idx), V(d_fuse_dist), V(d_nfused), V(stream or 0)),
           "plvi_fuse_lines_batch")


def distinctive_descriptors_batch(n_feat, d_pool, pool_rows, d_obs_off, d_obs_row, max_obs, d_best_pos, d_best_median,
                                  d_out_desc=0, stream=None):
    """MapPoint / MapLine::ComputeDistinctiveDescriptors over device tables (plvi_distinctive_descriptors_batch).
    d_pool: pool_rows descriptor rows of 32 bytes (e.g. the keyframes' device tables back to back); d_obs_off
    [n_feat + 1], d_obs_row: the CSR observation lists (pool rows in the caller's order; a row outside the pool is
    ignored); max_obs: the clamp of every list length (<= DISTINCTIVE_MAX_OBS).  Outputs d_best_pos, d_best_median
    [n_feat] (-1 / -1 where no entry remains) and d_out_desc [n_feat][32] (0 = not wanted; a row is written only
    where best_pos >= 0).  Asynchronous on `stream`."""
    V = ctypes.c_void_p
    _check(load().plvi_distinctive_descriptors_batch(n_feat, V(d_pool or 0), pool_rows, V(d_obs_off), V(d_obs_row or 0),
                                                     max_obs, V(d_best_pos), V(d_best_median), V(d_out_desc or 0),
                                                     V(stream or 0)),
           "plvi_distinctive_descriptors_batch")


def distinctive_descriptors(pool, obs_off, obs_row, out_desc=None):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:330-404) / MapLine::ComputeDistinctiveDescriptors
    (src/MapLine.cc:264-331) from host arrays.  pool: n x 32 uint8 descriptor rows; obs_off [n_feat + 1]
    (non-decreasing), obs_row: per feature the pool rows of its observations in the reference's list order (a row
    outside [0, n) is ignored, e.g. -1 for an absent leftIndex / rightIndex).  Returns (count, best_pos, best_median,
    out_desc): per feature the position inside its list of the first row with the least median distance (ignored
    entries counted; -1 when none remains), that median, and the row itself -- rows of `out_desc` (n_feat x 32,
    default zeros) with best_pos = -1 are left as passed in; count = features with best_pos >= 0."""
    pool = np.ascontiguousarray(pool, np.uint8).reshape(-1, 32)
    off = np.ascontiguousarray(obs_off, np.int32)
    rows = np.ascontiguousarray(obs_row, np.int32)
    n_feat = len(off) - 1
    if n_feat < 0 or (n_feat > 0 and len(rows) < int(off[-1])):
        raise ValueError("obs_off: n_feat + 1 offsets into obs_row")
    out = np.zeros((max(n_feat, 0), 32), np.uint8) if out_desc is None else out_desc
    if out.dtype != np.uint8 or out.shape != (n_feat, 32) or not out.flags.c_contiguous:
        raise ValueError("out_desc: a C-contiguous n_feat x 32 uint8 array")
    bp, bm = np.full(max(n_feat, 1), -7, np.int32), np.full(max(n_feat, 1), -7, np.int32)
    n = _check(load().plvi_distinctive_descriptors(_ptr(pool), len(pool), _ptr(off), _ptr(rows), n_feat, _ptr(bp),
                                                   _ptr(bm), _ptr(out)), "plvi_distinctive_descriptors")
    return n, bp[:n_feat], bm[:n_feat], out


def line_search_init(desc1, desc2):
    """One pair from host arrays: returns (LineMatches as an n x 2 int array
    (query, train), (nn_mad, nn12_mad))."""
    n1, n2 = len(desc1), len(desc2)
    c1, c2 = max(n1, 1), max(n2, 1)
    d1 = np.zeros((c1, 32), np.uint8)
    d1[:n1] = desc1
    d2 = np.zeros((c2, 32), np.uint8)
    d2[:n2] = desc2
    b1, b2 = DeviceBuffer(d1.nbytes), DeviceBuffer(d2.nbytes)
    b1.upload(d1)
    b2.upload(d2)
    cnt = DeviceBuffer(16)
    cnt.upload(np.array([n1, n2, 0, 0], np.int32))
    scr = DeviceBuffer(16 * c1)
    pr = DeviceBuffer(8 * c1)
    mad = DeviceBuffer(16)
    line_search_init_batch(b1.ptr, cnt.ptr, c1, b2.ptr, cnt.ptr + 4, c2, 1, scr.ptr, pr.ptr, cnt.ptr + 8, mad.ptr)
    load().plvi_device_synchronize()
    n = int(cnt.download(np.zeros(4, np.int32))[2])
    return pr.download(np.zeros((c1, 2), np.int32))[:n], tuple(mad.download(np.zeros(2, np.float64)))


# ----------------------------------------------------------------- stereo
def pack_pyramid(levels):
    """mvImagePyramid (list of 2-D uint8 arrays) -> (concatenated bytes, offsets, widths, heights)."""
    off = np.zeros(len(levels), np.int64)
    o = 0
    for i, lv in enumerate(levels):
        off[i] = o
        o += lv.size
    buf = np.concatenate([np.ascontiguousarray(lv, np.uint8).ravel() for lv in levels])
    w = np.array([lv.shape[1] for lv in levels], np.int32)
    h = np.array([lv.shape[0] for lv in levels], np.int32)
    return buf, off, w, h


def ComputeStereoMatches(kpsL, descL, kpsR, descR, pyrL, pyrR, scale_factors, inv_scale_factors, mb, mbf):
    """Frame::ComputeStereoMatches (src/Frame.cc:1228-1406) for one rectified pair.  kps*: mvKeys /
    mvKeysRight (KEYPOINT_DTYPE), pyr*: mvImagePyramid of the left / right extractor.  Returns
    (nstereo, mvuRight, mvDepth)."""
    lib = load()
    kl = np.ascontiguousarray(kpsL).view(KEYPOINT_DTYPE)
    kr = np.ascontiguousarray(kpsR).view(KEYPOINT_DTYPE)
    dl = np.ascontiguousarray(descL, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(descR, np.uint8).reshape(-1, 32)
    bl, off, w, h = pack_pyramid(pyrL)
    br, off2, w2, h2 = pack_pyramid(pyrR)
    if not (np.array_equal(off, off2) and np.array_equal(w, w2) and np.array_equal(h, h2)):
        raise ValueError("left and right pyramids differ in geometry")
    sc = np.ascontiguousarray(scale_factors, np.float32)
    inv = np.ascontiguousarray(inv_scale_factors, np.float32)
    n = len(kl)
    ur = np.full(max(n, 1), -1, np.float32)
    dp = np.full(max(n, 1), -1, np.float32)
    k = _check(lib.plvi_stereo_match(_ptr(kl), _ptr(dl), n, _ptr(kr), _ptr(dr), len(kr), len(pyrL), _ptr(sc),
                                     _ptr(inv), _ptr(bl), _ptr(br), _ptr(off), _ptr(w), _ptr(h), float(mb),
                                     float(mbf), _ptr(ur), _ptr(dp)), "plvi_stereo_match")
    return k, ur[:n], dp[:n]


def stereo_match_batch(left, right, n_frames, mb, mbf, d_uright, d_depth, d_nstereo, d_err, stream=None):
    """plvi_stereo_match_batch on two ORBextractor handles (device outputs, asynchronous)."""
    _check(load().plvi_stereo_match_batch(left._h, right._h, n_frames, float(mb), float(mbf),
                                          ctypes.c_void_p(d_uright), ctypes.c_void_p(d_depth),
                                          ctypes.c_void_p(d_nstereo), ctypes.c_void_p(d_err),
                                          ctypes.c_void_p(stream or 0)), "plvi_stereo_match_batch")


def ComputeStereoMatches_Lines(klL, descL, klR, descR, klUn, width, height, mbf, range_hint=1):
    """Frame::ComputeStereoMatches_Lines (src/Frame.cc:1408-1492) for one pair: mvKeys_Line, mvKeysRight_Line,
    mvKeysUn_Line (KEYLINE_DTYPE), LBD descriptors.  Returns (nstereo, matches_12, mvDisparity_l (n x 2),
    mvDepth_l (n x 2), mvle_l (n x 3))."""
    lib = load()
    a = np.ascontiguousarray(klL).view(KEYLINE_DTYPE)
    b = np.ascontiguousarray(klR).view(KEYLINE_DTYPE)
    u = a if klUn is None else np.ascontiguousarray(klUn).view(KEYLINE_DTYPE)
    dl = np.ascontiguousarray(descL, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(descR, np.uint8).reshape(-1, 32)
    n = len(a)
    m = np.full(max(n, 1), -1, np.int32)
    disp = np.full((max(n, 1), 2), -1, np.float32)
    dep = np.full((max(n, 1), 2), -1, np.float32)
    le = np.zeros((max(n, 1), 3), np.float64)
    k = _check(lib.plvi_stereo_lines(_ptr(a), _ptr(dl), n, _ptr(b), _ptr(dr), len(b), _ptr(u), int(width),
                                     int(height), float(mbf), int(range_hint), _ptr(m), _ptr(disp), _ptr(dep),
                                     _ptr(le)), "plvi_stereo_lines")
    return k, m[:n], disp[:n], dep[:n], le[:n]


def stereo_lines_scratch_bytes(n_frames, capL, capR, idx_cap):
    return load().plvi_stereo_lines_scratch_bytes(n_frames, capL, capR, idx_cap)


def stereo_lines_batch(n_frames, d_klL, d_descL, d_nL, capL, d_klR, d_descR, d_nR, capR, d_klUn, width, height,
                       mbf, range_hint, idx_cap, d_scratch, scratch_bytes, d_m12, d_disp, d_depth, d_le, d_nstereo,
                       d_err, stream=None):
    """plvi_stereo_lines_batch on device keyline tables (asynchronous)."""
    V = ctypes.c_void_p
    _check(load().plvi_stereo_lines_batch(n_frames, V(d_klL), V(d_descL), V(d_nL), capL, V(d_klR), V(d_descR),
                                          V(d_nR), capR, V(d_klUn or 0), width, height, float(mbf), range_hint,
                                          idx_cap, V(d_scratch), scratch_bytes, V(d_m12), V(d_disp), V(d_depth),
                                          V(d_le), V(d_nstereo), V(d_err), V(stream or 0)), "plvi_stereo_lines_batch")


LOCAL_MAP_LDS_KF = 8192         # PLVI_LOCAL_MAP_LDS_KF: largest kf_cap whose vote histogram is kept in LDS
LOCAL_MAP_GROUP_ENTRIES = 2048  # PLVI_LOCAL_MAP_GROUP_ENTRIES: keyframe-table entries per workgroup of the list passes
LOCAL_MAP_MAX_GROUPS = 64       # PLVI_LOCAL_MAP_MAX_GROUPS
LOCAL_MAP_MAX_ENTRIES = 0x7f7f7f7f  # PLVI_LOCAL_MAP_MAX_ENTRIES: largest kf_cap * max(kp_cap, kl_cap)
LOCAL_MAP_ERR_KF, LOCAL_MAP_ERR_MP, LOCAL_MAP_ERR_ML = 1, 2, 4

_LM_V, _LM_I = ctypes.c_void_p, ctypes.c_int


class LocalMapKeyframes(ctypes.Structure):
    """plvi_local_map_keyframes (include/plvi_frontend.h); pointers as integers, 0 / None = NULL."""
    _fields_ = [("kf_cap", _LM_I), ("n_order", _LM_I), ("kp_cap", _LM_I), ("kl_cap", _LM_I)] + \
               [(k, _LM_V) for k in ("bad", "order", "covis", "child_off", "child", "parent", "prev_kf", "mp", "nmp",
                                     "ml", "nml")]


class LocalMapPool(ctypes.Structure):
    """plvi_local_map_pool: MapPoints (pos) or MapLines (sep) by id."""
    _fields_ = [("n", _LM_I)] + [(k, _LM_V) for k in ("bad", "obs_off", "obs_kf", "pos", "sep", "normal", "dist",
                                                      "desc")]


class LocalMapFrames(ctypes.Structure):
    """plvi_local_map_frames: the per-frame vote / seen tables."""
    _fields_ = [("vote_mp", _LM_V), ("n_vote_mp", _LM_V), ("vote_mp_cap", _LM_I),
                ("vote_ml", _LM_V), ("n_vote_ml", _LM_V), ("vote_ml_cap", _LM_I),
                ("seen_mp", _LM_V), ("n_seen_mp", _LM_V), ("seen_mp_cap", _LM_I),
                ("seen_ml", _LM_V), ("n_seen_ml", _LM_V), ("seen_ml_cap", _LM_I), ("last_kf", _LM_V)]


class LocalMapOutputs(ctypes.Structure):
    """plvi_local_map_outputs: the lists, their full lengths, the gathered frustum tables and err."""
    _fields_ = [("lkf_cap", _LM_I), ("lmp_cap", _LM_I), ("lml_cap", _LM_I)] + \
               [(k, _LM_V) for k in ("local_kf", "n_local_kf", "ref_kf", "local_mp", "n_local_mp", "local_ml",
                                     "n_local_ml", "mp_pos", "mp_normal", "mp_dist", "mp_in_flags", "mp_desc",
                                     "ml_sep", "ml_normal", "ml_dist", "ml_in_flags", "ml_desc", "err")]


def local_map_scratch_bytes(n_frames, kf_cap, mp_n, ml_n=0):
    return load().plvi_local_map_scratch_bytes(n_frames, kf_cap, mp_n, ml_n)


def local_map_batch(n_frames, kf, mp, ml, frames, out, d_scratch, scratch_bytes, stream=None):
    """Tracking::UpdateLocalMap[WithLines] of n_frames frames on device tables (plvi_local_map_batch): kf / mp / ml
    / frames / out are the four structs above holding device addresses (ml may be None).  Asynchronous on
    `stream`; returns the status (negative = refused, nothing launched)."""
    ref = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731
    return load().plvi_local_map_batch(n_frames, ref(kf), ref(mp), ref(ml), ref(frames), ref(out),
                                       ctypes.c_void_p(d_scratch or 0), scratch_bytes, ctypes.c_void_p(stream or 0))


_LM_ROWS = {"pos": (np.float32, 3), "sep": (np.float64, 6), "normal": (np.float32, 3), "dist": (np.float32, 2),
            "desc": (np.uint8, 32)}


class LocalMap:
    """Tracking::UpdateLocalMap() / UpdateLocalMapWithLines() (src/Tracking.cc:5304-5323) over resident tables.

    ``keyframes``: a dict of numpy arrays named as the fields of plvi_local_map_keyframes -- bad [kf_cap], order,
    mp [kf_cap][kp_cap], nmp, and optionally covis [kf_cap][10], child_off / child, parent, prev_kf, ml / nml
    (ml selects the points-and-lines functions).  ``points`` / ``lines``: dicts named as plvi_local_map_pool --
    bad, obs_off, obs_kf and optionally pos (points) / sep (lines), normal, dist, desc.

    ``update`` runs one frame through the synchronous host form; ``update_batch`` uploads the tables once (they
    stay resident in ``self.dev``) and runs plvi_local_map_batch."""

    def __init__(self, keyframes, points, lines=None):
        self._lib = load()
        kf = dict(keyframes)
        i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
        self.kf = {"bad": np.ascontiguousarray(kf["bad"], np.uint8)}
        for k in ("order", "covis", "child_off", "child", "parent", "prev_kf", "mp", "nmp", "ml", "nml"):
            if kf.get(k) is not None:
                self.kf[k] = i32(kf[k])
        self.kf_cap = len(self.kf["bad"])
        self.kp_cap = self.kf["mp"].shape[1] if "mp" in self.kf and self.kf["mp"].ndim == 2 else 0
        self.kl_cap = self.kf["ml"].shape[1] if "ml" in self.kf and self.kf["ml"].ndim == 2 else 0
        self.pools = [self._pool(points), None if lines is None else self._pool(lines)]
        self.dev = None

    @staticmethod
    def _pool(p):
        q = {"bad": np.ascontiguousarray(p["bad"], np.uint8), "obs_off": np.ascontiguousarray(p["obs_off"], np.int32),
             "obs_kf": np.ascontiguousarray(p["obs_kf"], np.int32)}
        for k, (dt, w) in _LM_ROWS.items():
            if p.get(k) is not None:
                q[k] = np.ascontiguousarray(p[k], dt).reshape(len(q["bad"]), w)
        return q

    def _structs(self, ptr):
        """The keyframe and pool structs; ptr(group, name) -> the address of that table or None."""
        kf = LocalMapKeyframes(self.kf_cap, len(self.kf.get("order", ())), self.kp_cap, self.kl_cap)
        for k in self.kf:
            setattr(kf, k, ptr("kf", k))
        pools = []
        for g, p in zip(("mp", "ml"), self.pools):
            if p is None:
                pools.append(None)
                continue
            s = LocalMapPool(len(p["bad"]))
            for k in p:
                setattr(s, k, ptr(g, k))
            pools.append(s)
        return kf, pools[0], pools[1]

    def _tables(self):
        t = {("kf", k): a for k, a in self.kf.items()}
        for g, p in zip(("mp", "ml"), self.pools):
            if p is not None:
                t.update({(g, k): a for k, a in p.items()})
        return t

    def update(self, vote_mp, vote_ml=None, seen_mp=None, seen_ml=None, last_kf=-1, lkf_cap=None, lmp_cap=None,
               lml_cap=None, counts=None):
        """One frame from host arrays (plvi_local_map).  vote_* are updated in place when they are int32 arrays.
        `counts` ({"vote_mp": n, ...}) overrides a table's count, which is its length otherwise (to pass values
        outside [0, capacity]).
        Returns a dict: local_kf, ref_kf, local_mp, local_ml, the gathered tables the pools have rows for
        (mp_pos, mp_normal, mp_dist, mp_in_flags, mp_desc, ml_sep, ...), the full counts n_local_* and err."""
        tabs = self._tables()
        kf, mp, ml = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        lines = "ml" in self.kf
        n_mp, n_ml = len(self.pools[0]["bad"]), len(self.pools[1]["bad"]) if self.pools[1] else 0
        caps = [self.kf_cap if lkf_cap is None else lkf_cap, n_mp if lmp_cap is None else lmp_cap,
                n_ml if lml_cap is None else lml_cap]
        keep = []

        def table(a, count):
            if a is None:
                return None, None, 0
            a = a if isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous else \
                np.ascontiguousarray(a, np.int32)
            n = np.array([len(a) if count is None else count], np.int32)
            keep.extend([a, n])
            return a.ctypes.data if len(a) else None, n.ctypes.data, len(a)
        fr = LocalMapFrames()
        for name, a in (("vote_mp", vote_mp), ("vote_ml", vote_ml), ("seen_mp", seen_mp), ("seen_ml", seen_ml)):
            p, n, cap = table(a, (counts or {}).get(name))
            if a is not None and p is None:  # an empty table: a valid pointer with count 0
                z = np.zeros(1, np.int32)
                keep.append(z)
                p = z.ctypes.data
            setattr(fr, name, p)
            setattr(fr, "n_" + name, n)
            setattr(fr, name + "_cap", cap)
        last = np.array([last_kf], np.int32)
        fr.last_kf = last.ctypes.data
        res = self._outputs(1, caps, lines, -1)
        out = LocalMapOutputs(*caps)
        for k, a in res.items():
            setattr(out, k, a.ctypes.data)
        rc = self._lib.plvi_local_map(ctypes.byref(kf), ctypes.byref(mp), None if ml is None else ctypes.byref(ml),
                                      ctypes.byref(fr), ctypes.byref(out))
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_local_map")
        r = {k: a[0] for k, a in res.items()}
        nk, npnt = min(r["n_local_kf"], caps[0]), min(r["n_local_mp"], caps[1])
        r["local_kf"], r["local_mp"] = r["local_kf"][:nk], r["local_mp"][:npnt]
        for k in list(r):
            if k.startswith("mp_"):
                r[k] = r[k][:npnt]
        if lines:
            nl = min(r["n_local_ml"], caps[2])
            r["local_ml"] = r["local_ml"][:nl]
            for k in list(r):
                if k.startswith("ml_"):
                    r[k] = r[k][:nl]
        return r

    def _outputs(self, B, caps, lines, fill, gathers=None):
        """Host arrays for every output, pre-filled so that unwritten cells show."""
        o = {"local_kf": np.full((B, max(caps[0], 1)), fill, np.int32), "n_local_kf": np.full(B, fill, np.int32),
             "ref_kf": np.full(B, fill, np.int32), "local_mp": np.full((B, max(caps[1], 1)), fill, np.int32),
             "n_local_mp": np.full(B, fill, np.int32), "err": np.full(B, fill, np.int32)}
        if lines:
            o["local_ml"] = np.full((B, max(caps[2], 1)), fill, np.int32)
            o["n_local_ml"] = np.full(B, fill, np.int32)
        for g, p, cap in (("mp", self.pools[0], caps[1]), ("ml", self.pools[1] if lines else None, caps[2])):
            if p is None:
                continue
            for k, (dt, w) in list(_LM_ROWS.items()) + [("in_flags", (np.uint8, 1))]:
                if (k == "in_flags" or k in p) and (gathers is None or k in gathers):
                    shape = (B, max(cap, 1), w) if w > 1 else (B, max(cap, 1))
                    o[f"{g}_{k}"] = np.full(shape, fill & 0x7f if dt == np.uint8 else fill, dt)
        return o

    def upload(self):
        """Make the keyframe tables and pools resident (self.dev: (group, name) -> DeviceBuffer)."""
        if self.dev is None:
            self.dev = {}
            for key, a in self._tables().items():
                self.dev[key] = DeviceBuffer(a.nbytes)
                self.dev[key].upload(a)
        return self.dev

    def update_batch(self, vote_mp, n_vote_mp, vote_ml=None, n_vote_ml=None, seen_mp=None, n_seen_mp=None,
                     seen_ml=None, n_seen_ml=None, last_kf=None, lkf_cap=None, lmp_cap=None, lml_cap=None,
                     gathers=None, fill=-7, stream=None, run=True):
        """plvi_local_map_batch from host per-frame tables [B][cap] with every output downloaded: a dict of the
        output arrays (whole, sentinel-filled with `fill` where nothing was written), the in/out vote tables
        ("vote_mp" / "vote_ml"), "rc" and "d" (the output DeviceBuffers, for a device-side consumer).  `gathers`
        limits the gathered tables (None = all the pools have rows for).  run=False returns a callable
        step(stream) and a fetch() instead, for graph capture."""
        dev = self.upload()
        kf, mp, ml = self._structs(lambda g, k: dev[(g, k)].ptr)
        lines = "ml" in self.kf
        vote_mp = np.ascontiguousarray(vote_mp, np.int32)
        B = vote_mp.shape[0]
        n_mp, n_ml = len(self.pools[0]["bad"]), len(self.pools[1]["bad"]) if self.pools[1] else 0
        caps = [self.kf_cap if lkf_cap is None else lkf_cap, n_mp if lmp_cap is None else lmp_cap,
                n_ml if lml_cap is None else lml_cap]
        fr, fbuf, host_in = LocalMapFrames(), {}, {}
        for name, a, n in (("vote_mp", vote_mp, n_vote_mp), ("vote_ml", vote_ml, n_vote_ml),
                           ("seen_mp", seen_mp, n_seen_mp), ("seen_ml", seen_ml, n_seen_ml)):
            if a is None:
                continue
            a, n = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(n, np.int32)
            host_in[name] = a
            for key, arr in ((name, a), ("n_" + name, n)):
                fbuf[key] = DeviceBuffer(arr.nbytes)
                fbuf[key].upload(arr)
                setattr(fr, key, fbuf[key].ptr)
            setattr(fr, name + "_cap", a.shape[1])
        if last_kf is not None:
            lk = np.ascontiguousarray(last_kf, np.int32)
            fbuf["last_kf"] = DeviceBuffer(lk.nbytes)
            fbuf["last_kf"].upload(lk)
            fr.last_kf = fbuf["last_kf"].ptr
        res = self._outputs(B, caps, lines, fill, gathers)
        out, obuf = LocalMapOutputs(*caps), {}
        for k, a in res.items():
            obuf[k] = DeviceBuffer(a.nbytes)
            obuf[k].upload(a)
            setattr(out, k, obuf[k].ptr)
        sb = local_map_scratch_bytes(B, self.kf_cap, n_mp, n_ml if lines else 0)
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return local_map_batch(B, kf, mp, ml if lines else None, fr, out, scratch.ptr, sb, s)

        def fetch(rc=0):
            _check(self._lib.plvi_device_synchronize(), "plvi_device_synchronize")
            for k, a in res.items():
                obuf[k].download(a)
            r = dict(res)
            for name in ("vote_mp", "vote_ml"):
                if name in host_in:
                    r[name] = fbuf[name].download(np.empty_like(host_in[name]))
            r.update(rc=rc, d=obuf, keep=(fbuf, scratch))
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))


COVIS_LDS_KF = 8192     # PLVI_COVIS_LDS_KF: largest kf_cap whose vote histogram is kept in LDS
COVIS_MAX_CONN = 2048   # PLVI_COVIS_MAX_CONN: largest conn_cap
COVIS_TH = 15           # PLVI_COVIS_TH: th of KeyFrame::UpdateConnections
COVIS_MAX_QUERIES = 65535  # PLVI_COVIS_MAX_QUERIES


class CovisKeyframes(ctypes.Structure):
    """plvi_covis_keyframes (include/plvi_frontend.h); pointers as integers, 0 / None = NULL."""
    _fields_ = [("kf_cap", _LM_I), ("n_order", _LM_I), ("kp_cap", _LM_I), ("kl_cap", _LM_I)] + \
               [(k, _LM_V) for k in ("bad", "order", "mp", "nmp", "ml", "nml", "map_id", "init_kf", "first_conn",
                                     "parent", "covis")]


class CovisOutputs(ctypes.Structure):
    """plvi_covis_outputs: one int per query each."""
    _fields_ = [(k, _LM_V) for k in ("n_counted", "n_conn", "kf_max", "w_max", "new_parent", "err")]


def covis_scratch_bytes(n_queries, kf_cap):
    return load().plvi_covis_scratch_bytes(n_queries, kf_cap)


_COVIS_KF = {"bad": np.uint8, "order": np.int32, "mp": np.int32, "nmp": np.int32, "ml": np.int32, "nml": np.int32,
             "map_id": np.int32, "init_kf": np.uint8, "first_conn": np.uint8, "parent": np.int32, "covis": np.int32}
_COVIS_OUT = tuple(k for k, _ in CovisOutputs._fields_)


class Covisibility:
    """The covisibility graph of KeyFrame::UpdateConnections[WithLines] (src/KeyFrame.cc:499-769) over resident
    tables (plvi_covis_*): per keyframe slot the weight map and the ordered list, kept on the device.

    ``set_tables(keyframes, points, lines=None)``: dicts of numpy arrays named as the fields of
    plvi_covis_keyframes (bad, order, mp, nmp and optionally ml / nml, map_id, init_kf, first_conn, parent, covis)
    and plvi_local_map_pool (bad, obs_off, obs_kf).  ``update_batch`` runs on device copies of them (``self.dev``;
    first_conn / parent / covis are updated there, ``table(name)`` downloads one); ``update`` runs one keyframe
    through the synchronous host form and updates the host arrays in place."""

    def __init__(self, kf_cap, conn_cap, device=0):
        self._lib = load()
        h = ctypes.c_void_p()
        _check(self._lib.plvi_covis_create(kf_cap, conn_cap, device, ctypes.byref(h)), "plvi_covis_create")
        self.h, self.kf_cap, self.conn_cap = h, kf_cap, conn_cap
        self.kf, self.pools, self.dev = {}, [None, None], {}

    def close(self):
        if getattr(self, "h", None):
            self._lib.plvi_covis_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tables(self, keyframes, points, lines=None):
        self.kf = {k: np.ascontiguousarray(keyframes[k], dt) for k, dt in _COVIS_KF.items()
                   if keyframes.get(k) is not None}
        pool = lambda p: None if p is None else {  # noqa: E731
            "bad": np.ascontiguousarray(p["bad"], np.uint8), "obs_off": np.ascontiguousarray(p["obs_off"], np.int32),
            "obs_kf": np.ascontiguousarray(p["obs_kf"], np.int32)}
        self.pools = [pool(points), pool(lines)]
        self.dev = {}
        for key, a in self._tables().items():
            self.put(key[0], key[1], a)
        return self

    def _tables(self):
        t = {("kf", k): a for k, a in self.kf.items()}
        for g, p in zip(("mp", "ml"), self.pools):
            if p is not None:
                t.update({(g, k): a for k, a in p.items()})
        return t

    def put(self, group, name, a):
        """Replace one resident table (group "kf", "mp" or "ml")."""
        a = np.ascontiguousarray(a, _COVIS_KF[name] if group == "kf" else (np.uint8 if name == "bad" else np.int32))
        (self.kf if group == "kf" else self.pools[group == "ml"])[name] = a
        self.dev[(group, name)] = DeviceBuffer(a.nbytes)
        self.dev[(group, name)].upload(a)

    def table(self, name):
        """Download a keyframe table (first_conn, parent, covis, ...) from the device."""
        return self.dev[("kf", name)].download(np.empty_like(self.kf[name]))

    def _structs(self, ptr):
        shape = lambda k: self.kf[k].shape[1] if k in self.kf and self.kf[k].ndim == 2 else 0  # noqa: E731
        kf = CovisKeyframes(self.kf_cap, len(self.kf.get("order", ())), shape("mp"), shape("ml"))
        for k in self.kf:
            setattr(kf, k, ptr("kf", k))
        pools = []
        for g, p in zip(("mp", "ml"), self.pools):
            if p is None:
                pools.append(None)
                continue
            s = LocalMapPool(len(p["bad"]))
            for k in p:
                setattr(s, k, ptr(g, k))
            pools.append(s)
        return kf, pools[0], pools[1]

    def update_batch(self, q_slots, fill=-7, stream=None, run=True):
        """plvi_covis_update_batch of the keyframes q_slots, in that order.  Returns a dict of the per-query
        outputs (sentinel-filled with `fill` where nothing was written), "past" (the cell after the last query of
        each output: `fill` unless something wrote past the batch) and "rc".  run=False returns (step(stream),
        fetch()) instead, for graph capture."""
        q = np.ascontiguousarray(q_slots, np.int32)
        B = len(q)
        kf, mp, ml = self._structs(lambda g, k: self.dev[(g, k)].ptr)
        res = {k: np.full(B + 1, fill, np.int32) for k in _COVIS_OUT}   # one cell more than is written
        out, obuf = CovisOutputs(), {}
        for k, a in res.items():
            obuf[k] = DeviceBuffer(a.nbytes)
            obuf[k].upload(a)
            setattr(out, k, obuf[k].ptr)
        sb = covis_scratch_bytes(B, self.kf_cap)
        scratch = DeviceBuffer(sb)
        ref = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731

        def step(s=None):
            return self._lib.plvi_covis_update_batch(self.h, B, _ptr(q), ref(kf), ref(mp), ref(ml), ref(out),
                                                     ctypes.c_void_p(scratch.ptr), sb, ctypes.c_void_p(s or 0))

        def fetch(rc=0):
            _check(self._lib.plvi_device_synchronize(), "plvi_device_synchronize")
            r = {k: obuf[k].download(a)[:B] for k, a in res.items()}
            r.update(rc=rc, past=[int(a[B]) for a in res.values()], keep=(scratch, q))
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def update(self, slot):
        """One keyframe through the host form (plvi_covis_update): the host arrays first_conn / parent / covis
        given to set_tables are updated in place.  Returns the dict of outputs (ints) and "rc"."""
        tabs = self._tables()
        kf, mp, ml = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        res = {k: np.full(1, -7, np.int32) for k in _COVIS_OUT}
        out = CovisOutputs(*[a.ctypes.data for a in res.values()])
        rc = self._lib.plvi_covis_update(self.h, int(slot), ctypes.byref(kf), ctypes.byref(mp),
                                         None if ml is None else ctypes.byref(ml), ctypes.byref(out))
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_covis_update")
        r = {k: int(a[0]) for k, a in res.items()}
        r["rc"] = rc
        return r

    def _slots_call(self, fn, slots, stream):
        s = np.ascontiguousarray(slots, np.int32)
        cov = self.dev.get(("kf", "covis"))
        return fn(self.h, len(s), _ptr(s), ctypes.c_void_p(self.dev[("kf", "bad")].ptr),
                  ctypes.c_void_p(self.dev[("kf", "order")].ptr), len(self.kf["order"]),
                  ctypes.c_void_p(cov.ptr if cov else 0), ctypes.c_void_p(stream or 0))

    def erase(self, slots, stream=None):
        """The connection part of SetBadFlag for `slots` (plvi_covis_erase_batch); returns the status."""
        return self._slots_call(self._lib.plvi_covis_erase_batch, slots, stream)

    def resort(self, slots, stream=None):
        """UpdateBestCovisibles of `slots` (plvi_covis_resort_batch); returns the status."""
        return self._slots_call(self._lib.plvi_covis_resort_batch, slots, stream)

    def _pairs(self, fn, a, b, what):
        a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
        assert a.shape == b.shape
        da, db, do = DeviceBuffer(a.nbytes), DeviceBuffer(b.nbytes), DeviceBuffer(a.nbytes)
        da.upload(a)
        db.upload(b)
        _check(fn(self.h, len(a), ctypes.c_void_p(da.ptr), ctypes.c_void_p(db.ptr), ctypes.c_void_p(do.ptr), None), what)
        _check(self._lib.plvi_device_synchronize(), "plvi_device_synchronize")
        return do.download(np.empty_like(a))

    def by_weight(self, slots, weights):
        """len(GetCovisiblesByWeight(w)) per (slot, w)."""
        return self._pairs(self._lib.plvi_covis_by_weight_batch, slots, weights, "plvi_covis_by_weight_batch")

    def weight(self, a, b):
        """a->GetWeight(b) per pair of slots."""
        return self._pairs(self._lib.plvi_covis_weight_batch, a, b, "plvi_covis_weight_batch")

    def rows(self):
        """(ord_kf, ord_w, ord_n) device addresses of the ordered tables [kf_cap][conn_cap] and their counts."""
        p = [ctypes.c_void_p() for _ in range(3)]
        c = ctypes.c_int()
        _check(self._lib.plvi_covis_rows(self.h, *[ctypes.byref(x) for x in p], ctypes.byref(c)), "plvi_covis_rows")
        return tuple(x.value for x in p)

    def download(self, slot, fill=-7):
        """One slot's state: dict(map_kf, map_w (ascending slot), ord_kf, ord_w (as stored), err).  The arrays are
        conn_cap + 1 long and sentinel-filled past their counts n_map / n_ord."""
        C = self.conn_cap
        t = {k: np.full(C + 1, fill, np.int32) for k in ("map_kf", "map_w", "ord_kf", "ord_w")}
        n = [ctypes.c_int() for _ in range(3)]
        _check(self._lib.plvi_covis_download(self.h, int(slot), _ptr(t["map_kf"]), _ptr(t["map_w"]), ctypes.byref(n[0]),
                                             _ptr(t["ord_kf"]), _ptr(t["ord_w"]), ctypes.byref(n[1]),
                                             ctypes.byref(n[2])), "plvi_covis_download")
        t.update(n_map=n[0].value, n_ord=n[1].value, err=n[2].value)
        return t
