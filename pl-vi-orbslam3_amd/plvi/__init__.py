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

The ABI layer (loading, the signatures parsed from include/plvi_frontend.h, DeviceBuffer and the marshalling
helpers the wrappers below are written in) is plvi/_abi.py.
"""
import ctypes

import numpy as np

from ._abi import (HEADER_PATH, KEYLINE_DTYPE, KEYPOINT_DTYPE, LIB_PATH, PLVI_E_BADARG, PLVI_E_CAPACITY,  # noqa: F401
                   PLVI_E_CAPTURE, PLVI_E_EMPTY, PLVI_E_HIP, PLVI_E_OVERFLOW, PLVI_E_SIZE, PLVI_OK, DeviceBuffer,
                   PlviError, _check, _declare, _ptr, bound_runtime, c_int_p, c_void_pp, download,
                   exported_symbols, load, signatures)
from ._abi import (call as _call, out as _out, same_len as _same_len, status as _status, table as _table,
                   to_device as _to_device)

# OpenCV-semantics switches (plvi_frontend.h PLVI_COMPAT_*)
COMPAT_GAUSS_ROUNDED = 1
COMPAT_RESIZE_V_GENERIC = 2
COMPAT_EXP_CV_TABLE = 4


def _desc(a):
    """An n x 32 uint8 descriptor table (None stays None)."""
    return _table(a, np.uint8, 32)


def _sync():
    _call("plvi_device_synchronize")


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
    xy = _table(xy, np.float32, 2)
    n = len(xy)
    (d_in,), _ = _to_device(xy)
    d_out = DeviceBuffer(max(xy.nbytes, 8))
    _call("plvi_undistort_points", cam, d_in.ptr, n, d_out.ptr, None)
    _sync()
    return d_out.download(np.zeros((n, 2), np.float32))


def image_bounds(cam, cols, rows):
    """Frame::ComputeImageBounds (src/Frame.cc:1199-1226): (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    b = np.zeros(4, np.float32)
    _call("plvi_image_bounds", cam, cols, rows, b)
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


def frustum_params_init(p):
    """plvi_frustum_params_init: PredictScale's level_ratio table from nlevels / log_scale_factor."""
    _call("plvi_frustum_params_init", p)
    return p


def frustum_points(params, pos, normal, dist, in_flags, proj=None, level=None, depth=None, proj_r=None,
                   level_r=None):
    """Frame::isInFrustum over one frame's local MapPoints (src/Frame.cc:758-847) from host memory.
    proj / level / depth (/ proj_r / level_r) are the MapPoint fields on entry (stale values are kept
    where the reference keeps them).  Returns (nToMatch, flags, proj, level, depth, proj_r, level_r)."""
    pos = _table(pos, np.float32, 3)
    n = len(pos)
    nr, ds, fi = _table(normal, np.float32, 3), _table(dist, np.float32, 2), _table(in_flags, np.uint8)
    pr = np.zeros((n, 4), np.float32) if proj is None else np.array(proj, np.float32).reshape(-1, 4)
    lv = np.zeros(n, np.int32) if level is None else np.array(level, np.int32)
    de = np.zeros(n, np.float32) if depth is None else np.array(depth, np.float32)
    two = bool(params.two_camera)
    prr = (np.zeros((n, 4), np.float32) if proj_r is None else np.array(proj_r, np.float32).reshape(-1, 4)) \
        if two else None
    lvr = (np.zeros(n, np.int32) if level_r is None else np.array(level_r, np.int32)) if two else None
    _same_len(n, normal=nr, dist=ds, in_flags=fi, proj=pr, level=lv, depth=de, proj_r=prr, level_r=lvr)
    fo = _out(n, 0, np.uint8)
    nv = _call("plvi_frustum_points", params, pos, nr, ds, fi, n, fo, pr, lv, prr, lvr, de)
    return nv, fo[:n], pr, lv, de, prr, lvr


def frustum_lines(params, sep, normal, dist, in_flags, desc=None, proj=None, angle=None):
    """Frame::isInFrustum_l over one frame's local MapLines (src/Frame.cc:849-933) from host memory.
    Returns (inview, proj, angle, compact, compact_desc): compact = mvpLocalMapLines_InFrustum as local
    indices, compact_desc = their descriptors (None without desc)."""
    sp = _table(sep, np.float64, 6)
    n = len(sp)
    nr, ds, fi = _table(normal, np.float32, 3), _table(dist, np.float32, 2), _table(in_flags, np.uint8)
    de = _desc(desc)
    pr = np.zeros((n, 4), np.float32) if proj is None else np.array(proj, np.float32).reshape(-1, 4)
    an = np.zeros(n, np.float64) if angle is None else np.array(angle, np.float64)
    _same_len(n, normal=nr, dist=ds, in_flags=fi, desc=de, proj=pr, angle=an)
    iv, cp, cd = _out(n, 0, np.uint8), _out(n, 0), _out(n, 0, np.uint8, 32)
    nc = _call("plvi_frustum_lines", params, sp, nr, ds, fi, de, n, iv, pr, an, cp, cd)
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


def _output_cap(name, h):
    """The per-frame capacity plvi_orb_outputs / plvi_lines_outputs report."""
    cap = ctypes.c_int()
    _status(name, h, None, None, None, None, ctypes.byref(cap))
    return cap.value


def _outputs(name, h):
    """The four device pointers and the per-frame capacity of plvi_orb_outputs / plvi_lines_outputs."""
    p = [ctypes.c_void_p() for _ in range(4)]
    cap = ctypes.c_int()
    _call(name, h, *[ctypes.byref(x) for x in p], ctypes.byref(cap))
    return tuple(x.value for x in p) + (cap.value,)


def _errors(name, h, max_batch, stream, per_frame):
    flags = np.zeros(max_batch, np.int32)
    anyf = ctypes.c_int()
    _call(name, h, flags, ctypes.byref(anyf), stream or None)
    return flags if per_frame else anyf.value


def _sized_plane(name, h, frame, level, shape, dtype):
    """The two-call pattern of the pyramid / debug readers: ask for (w, h), then fill an array of shape(h, w)."""
    w, hgt = ctypes.c_int(), ctypes.c_int()
    _call(name, h, frame, level, None, ctypes.byref(w), ctypes.byref(hgt))
    plane = np.zeros(shape(hgt.value, w.value), dtype)
    _call(name, h, frame, level, plane, None, None)
    return plane


def _timing_read(name, h, kind):
    tot, n = ctypes.c_float(), ctypes.c_int()
    _call(name, h, int(kind), ctypes.byref(tot), ctypes.byref(n))
    return tot.value, n.value


def _profile_read(name, h, stages):
    ms = np.zeros(len(stages), np.float32)
    runs = ctypes.c_int()
    _call(name, h, ms, ctypes.byref(runs))
    return dict(zip(stages, ms.tolist())), runs.value


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
        _call("plvi_orb_create", self.params, width, height, max_batch, device, ctypes.byref(h))
        self._h = h
        self._refresh_cap()

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
        rc = _status("plvi_orb_extract", self._h, image if image.size else None, w, h, w, int(vLappingArea[0]),
                     int(vLappingArea[1]), kps, desc, self.kp_cap, ctypes.byref(n), ctypes.byref(mono))
        if rc == PLVI_E_EMPTY:
            return -1, np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
        if rc == PLVI_E_CAPACITY:  # a re-planned (larger) frame: grow the host buffers once
            self._refresh_cap()
            return self(image, mask, vLappingArea)
        _check(rc, "plvi_orb_extract")
        self._refresh_cap()
        return mono.value, kps[:n.value].copy(), desc[:n.value].copy()

    def _refresh_cap(self):
        self.kp_cap = _output_cap("plvi_orb_outputs", self._h)

    def errors(self, stream=None, per_frame=False):
        """Read-and-clear device error flags of the batches run so far (PLVI_FERR_*)."""
        return _errors("plvi_orb_errors", self._h, self.max_batch, stream, per_frame)

    # --- batched device path (bench / multi-frame) ---------------------------
    def extract_batch(self, d_frames_ptr, n_frames, frame_stride, row_stride, lap=(0, 0), stream=None):
        _call("plvi_orb_extract_batch", self._h, d_frames_ptr, n_frames, frame_stride, row_stride, lap[0], lap[1],
              stream or None)

    def outputs(self):
        """Device pointers (kps, desc, count, mono) and per-frame capacity."""
        return _outputs("plvi_orb_outputs", self._h)

    ORB_STAGES = ("level", "nms", "sat", "octree", "best", "describe", "assemble")

    def profile(self, enable=True):
        _call("plvi_orb_profile", self._h, int(enable))

    def profile_read(self):
        return _profile_read("plvi_orb_profile_read", self._h, self.ORB_STAGES)

    def kernel_timing(self, enable=True):
        """Event pair around every blur + FAST and pyramid kernel launch (rooflines)."""
        _call("plvi_orb_kernel_timing", self._h, int(enable))

    def kernel_timing_read(self, kind=0):
        """(total ms, launches) since kernel_timing(True): kind 0 = orb_blur_fast_kernel, 1 = orb_pyramid_kernel."""
        return _timing_read("plvi_orb_kernel_timing_read_kind", self._h, kind)

    # --- reference getters ---------------------------------------------------
    def _tables(self):
        tabs = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        _call("plvi_orb_scale_tables", self._h, *tabs)
        return tabs

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
        _call("plvi_orb_level_quota", self._h, q)
        return q

    def pyramid_level(self, level, frame=0):
        """mvImagePyramid[level] of the last call (lazy D2H)."""
        return _sized_plane("plvi_orb_pyramid_level", self._h, frame, level, lambda h, w: (h, w), np.uint8)

    @property
    def mvImagePyramid(self):
        return [self.pyramid_level(l) for l in range(self.nlevels)]

    def pyramid_device(self, level):
        """Device view of mvImagePyramid[level]: (frame-0 pointer, frame stride, w, h)."""
        p, fs = ctypes.c_void_p(), ctypes.c_size_t()
        w, h = ctypes.c_int(), ctypes.c_int()
        _call("plvi_orb_pyramid_device", self._h, level, ctypes.byref(p), ctypes.byref(fs), ctypes.byref(w),
              ctypes.byref(h), None)
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
        _call("plvi_lines_create", self.params, width, height, max_batch, device, ctypes.byref(h))
        self._h = h
        self.cap = _output_cap("plvi_lines_outputs", self._h)

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
        _call("plvi_lines_extract", self._h, image, w, h, w, kl, desc, fn, self.cap, ctypes.byref(n))
        self.width, self.height = w, h
        k = n.value
        return kl[:k].copy(), desc[:k].copy(), fn[:k].copy()

    def errors(self, stream=None, per_frame=False):
        """Read-and-clear device error flags of the batches run so far (PLVI_FERR_*)."""
        return _errors("plvi_lines_errors", self._h, self.max_batch, stream, per_frame)

    def extract_batch(self, d_frames_ptr, n_frames, frame_stride, row_stride, stream=None):
        _call("plvi_lines_extract_batch", self._h, d_frames_ptr, n_frames, frame_stride, row_stride, stream or None)

    def outputs(self):
        return _outputs("plvi_lines_outputs", self._h)

    def profile(self, enable=True):
        _call("plvi_lines_profile", self._h, int(enable))

    def profile_read(self):
        return _profile_read("plvi_lines_profile_read", self._h, self.STAGES)

    def kernel_timing(self, enable=True):
        """Event pair around every lsd_prep_kernel and LBD Gaussian + Sobel launch (rooflines)."""
        _call("plvi_lines_kernel_timing", self._h, int(enable))

    def kernel_timing_read(self, kind=0):
        """(total ms, launches) since kernel_timing(True): kind 0 = lsd_prep_kernel, 1 = lbd_sobel0_kernel,
        2 = lbd_sobel1_kernel, 3 = lsd_rect_lanes_kernel (region2rect), 4 = lbd_describe_kernel."""
        return _timing_read("plvi_lines_kernel_timing_read_kind", self._h, kind)

    def pyramid_level(self, level, frame=0):
        return _sized_plane("plvi_lines_pyramid_level", self._h, frame, level, lambda h, w: (h, w), np.uint8)

    def debug_planes(self, level, frame=0):
        """(deg f32, modgrad f64, cos/sin f32 [h, w, 2]) LSD planes of the last batch (diagnostic)."""
        w, h = ctypes.c_int(), ctypes.c_int()
        _call("plvi_lines_debug_planes", self._h, frame, level, None, None, None, ctypes.byref(w), ctypes.byref(h))
        deg = np.zeros((h.value, w.value), np.float32)
        mg = np.zeros((h.value, w.value), np.float64)
        cs = np.zeros((h.value, w.value, 2), np.float32)
        _call("plvi_lines_debug_planes", self._h, frame, level, deg, mg, cs, None, None)
        return deg, mg, cs

    def debug_raw_lines(self, level, frame=0):
        """n x 4 float32 (x1, y1, x2, y2): region2rect's segments of the last batch, one per region (diagnostic)."""
        n = ctypes.c_int()
        _call("plvi_lines_debug_raw_lines", self._h, frame, level, None, 1 << 30, ctypes.byref(n))
        lines = _out(n.value, 0, np.float32, 4)
        _call("plvi_lines_debug_raw_lines", self._h, frame, level, lines, n.value, ctypes.byref(n))
        return lines[:n.value].copy()

    def debug_sobel(self, level, frame=0):
        """(dx, dy) int16 LBD Sobel planes of the last batch (diagnostic)."""
        g = _sized_plane("plvi_lines_debug_sobel", self._h, frame, level, lambda h, w: (h, w, 2), np.int16)
        return g[..., 0].copy(), g[..., 1].copy()

    def scale_tables(self):
        tabs = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        _call("plvi_lines_scale_tables", self._h, *tabs)
        return tabs


def hamming_knn2(q, t):
    """BFMatcher(NORM_HAMMING).knnMatch(q, t, 2) -> (idx0, d0, idx1, d1) arrays."""
    q, t = _desc(q), _desc(t)
    res = [np.zeros(len(q), np.int32) for _ in range(4)]
    _call("plvi_hamming_knn2", q, len(q), t, len(t), *res)
    return tuple(res)


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


def _line_pairs_one(batch, desc1, desc2, *has_line):
    """One pair through line_search_init_batch / line_search_triangulation_batch (has_line: the latter's two
    flag tables): (npairs, pairs n x 2, (nn_mad, nn12_mad))."""
    d1, d2 = _desc(desc1), _desc(desc2)
    n1, n2 = len(d1), len(d2)
    c1, c2 = max(n1, 1), max(n2, 1)
    flags = [_table(h, np.uint8) for h in has_line]
    for n, name, h in zip((n1, n2), ("has_line1", "has_line2"), flags):
        _same_len(n, **{name: h})
    (b1, b2, *bh), cnt = _to_device(d1, d2, *flags, counts=(n1, n2))
    scr, pr, mad = DeviceBuffer(16 * c1), DeviceBuffer(8 * c1), DeviceBuffer(16)
    batch(b1.ptr, cnt.ptr, c1, b2.ptr, cnt.ptr + 4, c2, 1, *[b.ptr for b in bh], scr.ptr, pr.ptr, cnt.ptr + 8, mad.ptr)
    _sync()
    n = int(cnt.download(np.zeros(4, np.int32))[2])
    return n, pr.download(np.zeros((c1, 2), np.int32))[:n], tuple(mad.download(np.zeros(2, np.float64)))


class LineMatcher:
    """ORB_SLAM3::LineMatcher static Hamming matchers (src/LineMatcher.cpp)."""

    @staticmethod
    def _inout(name, desc1, desc2, nnr, matches_12):
        d1, d2 = _desc(desc1), _desc(desc2)
        prev = np.zeros(0, np.int32) if matches_12 is None else _table(matches_12, np.int32)
        m = _out(max(len(d1), prev.size), -1)
        m[:prev.size] = prev
        n = _call(name, d1, len(d1), d2, len(d2), nnr, m, prev.size)
        return n, m[:len(d1)].copy()

    @staticmethod
    def matchNNR(desc1, desc2, nnr, matches_12=None):
        """LineMatcher::matchNNR (LineMatcher.cpp:41-61).  matches_12: the caller's
        existing vector (kept through resize(rows, -1) like the reference), or None."""
        return LineMatcher._inout("plvi_line_match_nnr_inout", desc1, desc2, nnr, matches_12)

    @staticmethod
    def match(desc1, desc2, nnr, matches_12=None):
        """LineMatcher::match(desc1, desc2, nnr, matches_12) (LineMatcher.cpp:92-111)."""
        return LineMatcher._inout("plvi_line_match_inout", desc1, desc2, nnr, matches_12)

    @staticmethod
    def SearchByProjection(params, cur_angle, cur_desc, grid, last_flags, last_x3dc, last_octave, ml_desc,
                           cur_blocked=None):
        """LineMatcher::SearchByProjection(CurrentFrame, LastFrame, grid, th, angth) (src/LineMatcher.cpp:274-372).
        params: LineProjParams; grid: grid[x][y] lists of current-line indices (grid_Line); last_x3dc: n x 6
        camera-frame endpoints.  Returns (count, match) with match[i2] = last-frame line index or -1."""
        ca, cd, cb = _table(cur_angle, np.float32), _desc(cur_desc), _table(cur_blocked, np.uint8)
        cols, rows, off, idx = grid_csr(grid)
        params.grid_cols, params.grid_rows = cols, rows
        fl, x3 = _table(last_flags, np.uint8), _table(last_x3dc, np.float32, 6)
        oc, md = _table(last_octave, np.int32), _desc(ml_desc)
        _same_len(len(ca), cur_desc=cd, cur_blocked=cb)
        _same_len(len(fl), last_x3dc=x3, last_octave=oc, ml_desc=md)
        m = _out(len(ca), -1)
        n = _call("plvi_line_search_projection", params, ca, cd, cb, len(ca), off, idx, fl, x3, oc, md, len(fl), m)
        return n, m[:len(ca)]

    @staticmethod
    def Fuse(params, keylines, kl_desc, flags, spc, epc, dist, dot, level, ml_desc):
        """LineMatcher::Fuse(pKF, vpMapLines, th) (src/LineMatcher.cpp:373-485) as a pure search.  params:
        FuseLineParams; keylines: pKF->mvKeys_Line (KEYLINE_DTYPE) with mDescriptors_l; per MapLine (list order):
        flags (bit0 = non-NULL and not bad), spc / epc (n x 3, Rcw*SP + tcw, Rcw*EP + tcw), dist (n x 3: |0.5*(SP+EP)
        - Ow|, min / max distance invariance), dot (float64, OM.dot(pn)), level (PredictScale), descriptor.  Returns
        (nfused, fuse_idx, fuse_dist): the accepted keyline index and its distance per MapLine, else -1 / -1."""
        kl, kd, fl = _table(keylines, KEYLINE_DTYPE), _desc(kl_desc), _table(flags, np.uint8)
        sp, ep, ds = _table(spc, np.float32, 3), _table(epc, np.float32, 3), _table(dist, np.float32, 3)
        dt, lv, md = _table(dot, np.float64), _table(level, np.int32), _desc(ml_desc)
        _same_len(len(kl), kl_desc=kd)
        _same_len(len(fl), spc=sp, epc=ep, dist=ds, dot=dt, level=lv, ml_desc=md)
        n = len(fl)
        oi, od = _out(n, -1), _out(n, -1)
        nf = _call("plvi_fuse_lines", params, kl, kd, len(kl), fl, sp, ep, ds, dt, lv, md, n, oi, od)
        return nf, oi[:n], od[:n]

    @staticmethod
    def SearchForTriangulation(desc1, desc2, has_line1, has_line2):
        """SearchForTriangulation(pKF1, pKF2, vMatchedPairs) (src/LineMatcher.cpp:142-171): has_line =
        GetMapLine(i) != NULL per line.  Returns (nmatches, vMatchedPairs as an n x 2 int array (query, train),
        (nn_mad, nn12_mad))."""
        return _line_pairs_one(line_search_triangulation_batch, desc1, desc2, has_line1, has_line2)

    @staticmethod
    def matchGrid(lines1, desc1, grid, desc2, directions2, window=((7, 0), (2, 2)), range_hint=1):
        """LineMatcher::matchGrid (src/LineMatcher.cpp:191-272).  lines1: n1 x 4 ints (line_2d grid coords),
        grid: grid[x][y] lists of right-line indices, directions2: n2 x 2.  range_hint: 1 = libstdc++ <= GCC 10
        candidate order (the reference's toolchain), 0 = GCC >= 11.  Returns (nmatches, matches_12)."""
        l1, d1 = _table(lines1, np.int32, 4), _desc(desc1)
        d2, v2 = _desc(desc2), _table(directions2, np.float64, 2)
        _same_len(len(l1), desc1=d1)
        _same_len(len(d2), directions2=v2)
        cols, rows, off, idx = grid_csr(grid)
        m = _out(len(l1), -1)
        (w0, w1), (h0, h1) = window
        n = _call("plvi_line_match_grid", l1, d1, len(l1), cols, rows, off, idx, d2, v2, len(d2), w0, w1, h0, h1,
                  int(range_hint), m)
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
        kd, ka, kl = _desc(kf_desc), _table(kf_angle, np.float32), _table(kf_live, np.uint8)
        fd, fa = _desc(f_desc), _table(f_angle, np.float32)
        _same_len(len(kd), kf_angle=ka, kf_live=kl)
        _same_len(len(fd), f_angle=fa)
        kn, ko, ki = feature_vector_csr(kf_featvec)
        fn, fo, fi = feature_vector_csr(f_featvec)
        m = _out(len(fd), -1)
        n = _call("plvi_search_by_bow_stereo", self.nnratio, int(self.check_orientation), kd, ka, kl, len(kd), kn, ko,
                  len(kn), ki, fd, fa, len(fd), fn, fo, len(fn), fi, int(f_nleft), m)
        return n, m[:len(fd)]

    def SearchByBoWKF(self, desc1, angle1, live1, featvec1, desc2, angle2, live2, featvec2):
        """SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
        (src/ORBmatcher.cc:823-963), single-camera branch.  Per side: mDescriptors, mvKeysUn angles, live[i] =
        GetMapPointMatches()[i] is non-NULL and not bad, mFeatVec as {node: [indices]}.  Returns (nmatches,
        matches12) with matches12[idx1] = the KF2 keypoint index whose MapPoint goes to vpMatches12[idx1], or -1."""
        d1, a1, l1 = _desc(desc1), _table(angle1, np.float32), _table(live1, np.uint8)
        d2, a2, l2 = _desc(desc2), _table(angle2, np.float32), _table(live2, np.uint8)
        n1, n2 = len(d1), len(d2)
        _same_len(n1, angle1=a1, live1=l1)
        _same_len(n2, angle2=a2, live2=l2)
        a, ao, ai = feature_vector_csr(featvec1)
        b, bo, bi = feature_vector_csr(featvec2)
        m = _out(n1, -1)
        n = _call("plvi_search_by_bow_kf", self.nnratio, int(self.check_orientation), d1, a1, l1, n1, a, ao, len(a),
                  ai, d2, a2, l2, n2, b, bo, len(b), bi, m)
        return n, m[:n1]

    def SearchForTriangulation(self, kps1, desc1, featvec1, has_point1, uright1, kps2, desc2, featvec2, has_point2,
                               uright2, F12, ep, sigma2, scale_factors, bOnlyStereo=False, bCoarse=False):
        """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse)
        (src/ORBmatcher.cc:965-1206), single-camera Pinhole branch.  Keypoints are mvKeysUn in
        KEYPOINT_DTYPE, has_point = GetMapPoint(i) != NULL, uright = mvuRight; F12 (3 x 3) and the epipole
        ep replace what the reference derives from the poses (plvi_frontend.h), sigma2 / scale_factors
        are pKF2's mvLevelSigma2 / mvScaleFactors.  Returns (nmatches, vMatchedPairs as an n x 2 int
        array (idx1, idx2) in idx1 order)."""
        k1, k2 = _table(kps1, KEYPOINT_DTYPE), _table(kps2, KEYPOINT_DTYPE)
        n1, n2 = len(k1), len(k2)
        d1, h1, u1 = _desc(desc1), _table(has_point1, np.uint8), _table(uright1, np.float32)
        d2, h2, u2 = _desc(desc2), _table(has_point2, np.uint8), _table(uright2, np.float32)
        _same_len(n1, desc1=d1, has_point1=h1, uright1=u1)
        _same_len(n2, desc2=d2, has_point2=h2, uright2=u2)
        a, ao, ai = feature_vector_csr(featvec1)
        b, bo, bi = feature_vector_csr(featvec2)
        pair = TriangulationPair.make(F12, ep, sigma2, scale_factors, bOnlyStereo, bCoarse, self.check_orientation)
        m = _out(n1, -1)
        n = _call("plvi_search_for_triangulation", pair, k1, d1, n1, a, ao, len(a), ai, h1, u1, k2, d2, n2, b, bo,
                  len(b), bi, h2, u2, m)
        m = m[:n1]
        i1 = np.flatnonzero(m >= 0)
        return n, np.stack([i1, m[i1]], axis=1).astype(np.int32)

    def SearchByProjection(self, params, cur_kps, cur_desc, last_x3dc, last_octave, last_angle, mp_desc,
                           last_flags, cur_blocked=None, cur_uright=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1962-2178) with
        mbCheckOrientation = checkOri of this matcher.  params: ProjParams (th, camera, grid, bounds,
        scale factors); cur_kps: mvKeysUn (KEYPOINT_DTYPE); last_*: see include/plvi_frontend.h.
        Returns (nmatches, match) with match[i2] = LastFrame index, -2 (nulled) or -1 (untouched)."""
        params.check_orientation = int(self.check_orientation)
        ck, cd = _table(cur_kps, KEYPOINT_DTYPE), _desc(cur_desc)
        cb, cu = _table(cur_blocked, np.uint8), _table(cur_uright, np.float32)
        x3, lo, la = _table(last_x3dc, np.float32, 3), _table(last_octave, np.int32), _table(last_angle, np.float32)
        md, lf = _desc(mp_desc), _table(last_flags, np.uint8)
        n = len(ck)
        _same_len(n, cur_desc=cd, cur_blocked=cb, cur_uright=cu)
        _same_len(len(lf), last_x3dc=x3, last_octave=lo, last_angle=la, mp_desc=md)
        m = _out(n, -1)
        nm = _call("plvi_search_by_projection", params, ck, cd, n, cb, cu, x3, lo, la, md, lf, len(lf), m)
        return nm, m[:n]

    def SearchByProjectionLocal(self, params, kps, desc, mp_flags, mp_proj, mp_level, mp_desc, blocked=None,
                                uright=None):
        """SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
        (src/ORBmatcher.cc:44-145, monocular / rectified branch) with this matcher's nnratio.  params:
        LocalParams (grid, th, scale factors); kps: F.mvKeysUn; mp_*: per MapPoint (vector order) flags (bit0
        searched, bit1 Observations() > 0), proj (n x 4: mTrackProjX, mTrackProjY, mTrackProjXR,
        mTrackViewCos), mnTrackScaleLevel, descriptor.  Returns (nmatches, match) with match[idx] = MapPoint
        index stored in F.mvpMapPoints[idx] or -1."""
        params.nnratio = self.nnratio
        k, d = _table(kps, KEYPOINT_DTYPE), _desc(desc)
        cb, cu = _table(blocked, np.uint8), _table(uright, np.float32)
        fl, pr = _table(mp_flags, np.uint8), _table(mp_proj, np.float32, 4)
        lv, md = _table(mp_level, np.int32), _desc(mp_desc)
        _same_len(len(k), desc=d, blocked=cb, uright=cu)
        _same_len(len(fl), mp_proj=pr, mp_level=lv, mp_desc=md)
        m = _out(len(k), -1)
        nm = _call("plvi_search_local", params, k, d, len(k), cb, cu, fl, pr, lv, md, len(fl), m)
        return nm, m[:len(k)]

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
        k, d, cb = _table(kps, KEYPOINT_DTYPE), _desc(desc), _table(blocked, np.uint8)
        kr, dr, cbr = _table(kps_r, KEYPOINT_DTYPE), _desc(desc_r), _table(blocked_r, np.uint8)
        x3, x3r = _table(x3dc, np.float32, 3), _table(x3dr, np.float32, 3)
        lo, la = _table(last_octave, np.int32), _table(last_angle, np.float32)
        md, lf, kb = _desc(mp_desc), _table(last_flags, np.uint8), _table(kb8, np.float32)
        _same_len(len(k), desc=d, blocked=cb)
        _same_len(len(kr), desc_r=dr, blocked_r=cbr)
        _same_len(len(lf), x3dc=x3, x3dr=x3r, last_octave=lo, last_angle=la, mp_desc=md)
        m, mr = _out(len(k), -1), _out(len(kr), -1)
        nm = _call("plvi_search_by_projection_stereo", params, kb, k, d, len(k), cb, kr, dr, len(kr), cbr, x3, x3r,
                   lo, la, md, lf, len(lf), m, mr)
        return nm, m[:len(k)], mr[:len(kr)]

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
        k, d = _table(kps, KEYPOINT_DTYPE), _desc(desc)
        kr, dr = _table(kps_r, KEYPOINT_DTYPE), _desc(desc_r)
        cb, a = _table(blocked, np.uint8), _table(l2r, np.int32)
        cbr, b = _table(blocked_r, np.uint8), _table(r2l, np.int32)
        fl, md = _table(mp_flags, np.uint8), _desc(mp_desc)
        pr, lv = _table(mp_proj, np.float32, 4), _table(mp_level, np.int32)
        prr, lvr = _table(mp_proj_r, np.float32, 4), _table(mp_level_r, np.int32)
        _same_len(len(k), desc=d, blocked=cb, l2r=a)
        _same_len(len(kr), desc_r=dr, blocked_r=cbr, r2l=b)
        _same_len(len(fl), mp_proj=pr, mp_level=lv, mp_proj_r=prr, mp_level_r=lvr, mp_desc=md)
        m, mr = _out(len(k), -1), _out(len(kr), -1)
        nm = _call("plvi_search_local_stereo", params, k, d, len(k), cb, a, kr, dr, len(kr), cbr, b, fl, pr, lv, prr,
                   lvr, md, len(fl), m, mr)
        return nm, m[:len(k)], mr[:len(kr)]

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
        ck, cd, cb = _table(cur_kps, KEYPOINT_DTYPE), _desc(cur_desc), _table(cur_blocked, np.uint8)
        fl, x3, ds = _table(kf_flags, np.uint8), _table(x3dc, np.float32, 3), _table(dist, np.float32, 3)
        lv, ka, md = _table(level, np.int32), _table(kf_angle, np.float32), _desc(mp_desc)
        n = len(ck)
        _same_len(n, cur_desc=cd, cur_blocked=cb)
        _same_len(len(fl), x3dc=x3, dist=ds, level=lv, kf_angle=ka, mp_desc=md)
        m = _out(n, -1)
        nm = _call("plvi_search_reloc", params, ck, cd, n, cb, fl, x3, ds, lv, ka, md, len(fl), m)
        return nm, m[:n]

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
        k, d, mb = _table(kps, KEYPOINT_DTYPE), _desc(desc), _table(matched, np.uint8)
        fl, x3, ds = _table(flags, np.uint8), _table(x3dc, np.float32, 3), _table(dist, np.float32, 3)
        dt, lv, md = _table(dot, np.float64), _table(level, np.int32), _desc(mp_desc)
        n = len(k)
        _same_len(n, desc=d, matched=mb)
        _same_len(len(fl), x3dc=x3, dist=ds, dot=dt, level=lv, mp_desc=md)
        m = _out(n, -1)
        nm = _call("plvi_search_sim3_projection", params, k, d, n, mb, fl, x3, ds, dt, lv, md, len(fl), m)
        return nm, m[:n]

    def _fuse(self, mode, params, kps, desc, flags, x3dc, dist, dot, level, mp_desc, uright):
        params.mode = mode
        k, d, ur = _table(kps, KEYPOINT_DTYPE), _desc(desc), _table(uright, np.float32)
        fl, x3, ds = _table(flags, np.uint8), _table(x3dc, np.float32, 3), _table(dist, np.float32, 3)
        dt, lv, md = _table(dot, np.float64), _table(level, np.int32), _desc(mp_desc)
        _same_len(len(k), desc=d, uright=ur)
        _same_len(len(fl), x3dc=x3, dist=ds, dot=dt, level=lv, mp_desc=md)
        n = len(fl)
        oi, od = _out(n, -1), _out(n, -1)
        nf = _call("plvi_fuse_points", params, k, d, len(k), ur, fl, x3, ds, dt, lv, md, n, oi, od)
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
        a, b = _desc(a), _desc(b)
        n = len(a)
        _same_len(n, b=b)
        (da, db), _ = _to_device(a, b)
        do = DeviceBuffer(max(4 * n, 4))
        _call("plvi_descriptor_distance_batch", da.ptr, db.ptr, n, int(line_matcher_quirk), do.ptr, None)
        _sync()
        return do.download(np.zeros(n, np.int32))


def frame_extract_batch(orb, lines, d_frames_ptr, n_frames, frame_stride, row_stride, lap=(0, 0), stream=None):
    """Frame::Frame's ORB + line extraction of a device batch as one schedule
    (plvi_frame_extract_batch); results via orb.outputs() / lines.outputs()."""
    _call("plvi_frame_extract_batch", orb._h, lines._h, d_frames_ptr, n_frames, frame_stride, row_stride, lap[0],
          lap[1], stream or None)


def frame_extract_match_batch(orb, lines, d_frames_ptr, n_frames, frame_stride, row_stride, knn_out, nnr,
                              line_scratch, line_matches, line_nmatch, lap=(0, 0), stream=None):
    """plvi_frame_extract_match_batch: the frame schedule plus the step's matching of frame t vs t-1 (ORB
    kNN-2 into knn_out = (idx0, d0, idx1, d1) device pointers, LineMatcher::match into line_matches /
    line_nmatch) issued inside the schedule's streams."""
    _call("plvi_frame_extract_match_batch", orb._h, lines._h, d_frames_ptr, n_frames, frame_stride, row_stride,
          lap[0], lap[1], *knn_out, float(nnr), line_scratch, line_matches, line_nmatch, stream or None)


def frame_orb_event(lines):
    """plvi_frame_orb_event: the hipEvent_t the last frame_extract_batch on `lines` recorded when its ORB
    part completed (handle-owned)."""
    e = ctypes.c_void_p()
    _call("plvi_frame_orb_event", lines._h, ctypes.byref(e))
    return e.value


def event_create():
    e = ctypes.c_void_p()
    _call("plvi_event_create", ctypes.byref(e))
    return e.value


def event_record(event, stream=None):
    _call("plvi_event_record", event, stream or None)


def stream_wait_event(stream, event):
    _call("plvi_stream_wait_event", stream or None, event)


def event_destroy(event):
    _call("plvi_event_destroy", event)


def stereo_frame_extract_batch(orb_left, orb_right, lines_left, lines_right, d_left_ptr, d_right_ptr, n_frames,
                               frame_stride, row_stride, lap=(0, 0), stream=None):
    """The stereo-line Frame's four extractions (plvi_stereo_frame_extract_batch)."""
    _call("plvi_stereo_frame_extract_batch", orb_left._h, orb_right._h, lines_left._h, lines_right._h, d_left_ptr,
          d_right_ptr, n_frames, frame_stride, row_stride, lap[0], lap[1], stream or None)


class StepGraph:
    """A batch step captured into a HIP graph (plvi_graph_*): ``fn(stream)``
    issues plvi_* calls on ``stream`` (a created stream); the graph replays
    them with one launch.  The captured pointers and parameters are fixed."""

    def __init__(self, fn, stream):
        self._lib = load()
        self._stream = stream
        _call("plvi_graph_capture_begin", stream)
        try:
            fn(stream)
        finally:
            ex = ctypes.c_void_p()
            rc = _status("plvi_graph_capture_end", stream, ctypes.byref(ex))
        _check(rc, "plvi_graph_capture_end")
        self._exec = ex

    def launch(self, stream=None):
        _call("plvi_graph_launch", self._exec, stream or self._stream)

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
        _call("plvi_vocab_info", self._h, info)
        self.k, self.L, self.scoring, self.weighting, self.n_nodes, self.n_words = (int(x) for x in info)

    @classmethod
    def loadFromTextFile(cls, path, emulate_tail=False, device=0):
        """TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1424).  emulate_tail=True adds
        the node the reference's `while(!f.eof()) getline` loop reads from the empty tail after a final
        newline -- undefined in the reference (pid / nIsLeaf / the descriptor stay unassigned), modelled here
        as a zero-descriptor non-word child of the root; off by default."""
        h = ctypes.c_void_p()
        _call("plvi_vocab_load_text", str(path).encode(), int(emulate_tail), device, ctypes.byref(h))
        return cls(h)

    @classmethod
    def from_nodes(cls, k, L, scoring, weighting, parent, is_leaf, desc, weight, device=0):
        parent, is_leaf = _table(parent, np.int32), _table(is_leaf, np.uint8)
        desc, weight = _desc(desc), _table(weight, np.float64)
        h = ctypes.c_void_p()
        _call("plvi_vocab_create", k, L, scoring, weighting, len(parent), parent, is_leaf, desc, weight, device,
              ctypes.byref(h))
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
        d = _desc(desc)
        n = len(d)
        bw, bv = _out(n, 0, np.uint32), _out(n, 0, np.float64)
        fn, fo, fi = _out(n, 0, np.uint32), _out(n + 1, 0), _out(n, 0, np.uint32)
        nb, nf = ctypes.c_int(), ctypes.c_int()
        _call("plvi_vocab_transform", self._h, d, n, levelsup, bw, bv, ctypes.byref(nb), fn, fo, fi, ctypes.byref(nf))
        nb, nf = nb.value, nf.value
        return bw[:nb], bv[:nb], fn[:nf], fo[:nf + 1], fi[:fo[nf]]

    def transform(self, desc, levelsup=4):
        bw, bv, fn, fo, fi = self.transform_arrays(desc, levelsup)
        bow = {int(w): float(v) for w, v in zip(bw, bv)}
        fv = {int(fn[i]): [int(x) for x in fi[fo[i]:fo[i + 1]]] for i in range(len(fn))}
        return bow, fv

    def transform_features(self, desc, levelsup=4):
        """Per-descriptor (word ids, node ids at level L - levelsup)."""
        d = _desc(desc)
        n = len(d)
        w, ni = _out(n, 0, np.uint32), _out(n, 0, np.uint32)
        _call("plvi_vocab_transform_features", self._h, d, n, levelsup, w, ni)
        return w[:n], ni[:n]


def _bow_arrays(bow):
    """A BowVector as (ascending uint32 words, float64 values): a {word: value} dict or a (words, values) pair."""
    if isinstance(bow, dict):
        ws = sorted(bow)
        return np.array(ws, np.uint32), np.array([bow[w] for w in ws], np.float64)
    w, v = bow
    return _table(w, np.uint32), _table(v, np.float64)


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
    e = _table(entries, np.int32, 3)
    _call("plvi_kfdb_add_batch", db._h, len(e), e, d_bow_word or None, d_bow_value or None, d_bow_n, cap,
          stream or None)


def kfdb_query_batch(db, n_queries, d_q_word, d_q_value, d_q_n, q_cap, d_q_map, mode, n_best=3, d_conn_off=0,
                     d_conn_slot=0, d_covis=0, d_map_bad=0, n_maps=0, d_words=0, d_score=0, d_order=0, d_norder=0,
                     d_cand=0, cand_cap=0, d_ncand=0, d_loop=0, d_nloop=0, d_merge=0, d_nmerge=0, stream=None):
    """DetectRelocalizationCandidates (mode 0) / DetectNBestCandidates (mode 1) of n_queries device BowVectors
    (plvi_kfdb_query_batch; every pointer is a device address, 0 = NULL).  Asynchronous on `stream`."""
    _call("plvi_kfdb_query_batch", db._h, n_queries, d_q_word or None, d_q_value or None, d_q_n, q_cap, d_q_map, mode,
          n_best, d_conn_off or None, d_conn_slot or None, d_covis or None, d_map_bad or None, n_maps,
          d_words or None, d_score or None, d_order or None, d_norder or None, d_cand or None, cand_cap,
          d_ncand or None, d_loop or None, d_nloop or None, d_merge or None, d_nmerge or None, stream or None)


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
        _call("plvi_kfdb_create", n_words, slot_cap, word_cap, scoring, device, ctypes.byref(h))
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
        _same_len(len(w), value=v)
        _call("plvi_kfdb_add", self._h, slot, map_id, w, v, len(w))

    def add_many(self, slots, bows, map_ids):
        """add of several keyframes in the given order through plvi_kfdb_add_batch."""
        word, value, n = pack_bow(bows)
        bufs, _ = _to_device(word, value, n)
        entries = np.stack([np.arange(len(slots)), np.asarray(slots), np.asarray(map_ids)], axis=1)
        kfdb_add_batch(self, entries, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, word.shape[1])
        return self.errors()

    def erase(self, slots, stream=None):
        s = np.atleast_1d(np.asarray(slots, np.int32))
        _call("plvi_kfdb_erase", self._h, len(s), s, stream or None)

    def clearMap(self, map_id, stream=None):
        _call("plvi_kfdb_clear_map", self._h, map_id, stream or None)

    def clear(self, stream=None):
        _call("plvi_kfdb_clear", self._h, stream or None)

    def errors(self, stream=None):
        """Read and clear the error word (bit 0: a count above word_cap, bit 1: a word id >= n_words)."""
        f = ctypes.c_int()
        _status("plvi_kfdb_errors", self._h, ctypes.byref(f), stream or None)
        return f.value

    def _covis(self, covis):
        c = _table(covis, np.int32)
        if c is not None and c.shape != (self.slot_cap, KFDB_NEIGHBOURS):
            raise ValueError("covis: slot_cap x 10 slots, -1 ends a row")
        return c

    def DetectRelocalizationCandidates(self, bow, map_id, covis=None, cand_cap=None):
        """vpRelocCandidates as slots, in the reference's order (KeyFrameDatabase.cc:790-902)."""
        w, v = _bow_arrays(bow)
        _same_len(len(w), value=v)
        c = self._covis(covis)
        cap = self.slot_cap if cand_cap is None else cand_cap
        cand = _out(cap, -1)
        n = _call("plvi_kfdb_query", self._h, w, v, len(w), map_id, 0, 0, None, 0, c, None, 0, cand, cap, None, None,
                  None, None)
        return [int(x) for x in cand[:min(n, cap)]]

    def DetectNBestCandidates(self, bow, map_id, connected=(), n_best=3, covis=None, map_bad=None):
        """(vpLoopCand, vpMergeCand) as slots (KeyFrameDatabase.cc:619-787)."""
        w, v = _bow_arrays(bow)
        _same_len(len(w), value=v)
        c = self._covis(covis)
        conn = np.ascontiguousarray(sorted(connected), np.int32)
        bad = _table(map_bad, np.uint8)
        loop, merge = _out(n_best, -1), _out(n_best, -1)
        nl, nm = ctypes.c_int(), ctypes.c_int()
        _call("plvi_kfdb_query", self._h, w, v, len(w), map_id, 1, n_best, conn if len(conn) else None, len(conn), c,
              bad, 0 if bad is None else len(bad), None, 0, loop, ctypes.byref(nl), merge, ctypes.byref(nm))
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
            n = _table(counts, np.int32)
        c = self._covis(covis)
        conn = [sorted(x) for x in connected] if connected is not None else None
        ins = {"word": word, "value": value, "n": n, "map": _table(map_ids, np.int32)}
        if conn is not None:
            off = np.zeros(nq + 1, np.int32)
            off[1:] = np.cumsum([len(x) for x in conn])
            ins["coff"], ins["cslot"] = off, np.array([s for x in conn for s in x] + [0], np.int32)
        if c is not None:
            ins["covis"] = c
        if map_bad is not None:
            ins["bad"] = _table(map_bad, np.uint8)
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
        _sync()
        for k, a in outs.items():
            d[k].download(a)
        return outs


def assign_grid_batch(d_kps, d_count, cap, n_frames, grid, d_cell_off, d_cell_idx, stream=None):
    """Frame::AssignFeaturesToGrid (src/Frame.cc:644-675) of device keypoint tables -> CSR grids."""
    _call("plvi_assign_grid_batch", d_kps, d_count, cap, n_frames, grid, d_cell_off, d_cell_idx, stream or None)


# ------------------------------------------------------- initialization
def search_for_initialization_batch(n_pairs, params, d_kps1, d_desc1, d_n1, cap1, d_prev, d_kps2, d_desc2, d_n2, cap2,
                                    d_cell_off, d_cell_idx, d_m12, d_nm, stream=None):
    """ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:705-814) over device pair tables."""
    _call("plvi_search_for_initialization_batch", n_pairs, params, d_kps1, d_desc1, d_n1, cap1, d_prev, d_kps2,
          d_desc2, d_n2, cap2, d_cell_off, d_cell_idx, d_m12, d_nm, stream or None)


def search_for_initialization(kps1, desc1, prev_xy, kps2, desc2, width=640, height=480, window=100, nnratio=0.9,
                              check_orientation=True, grid=None):
    """One (F1, F2) pair from host arrays (keypoints in KEYPOINT_DTYPE = mvKeysUn,
    descriptors n x 32, prev_xy = vbPrevMatched n1 x 2): returns (nmatches,
    vnMatches12, updated vbPrevMatched).  grid = (min_x, min_y, inv_w, inv_h)
    (default: the Frame grid of an undistorted width x height image)."""
    if grid is None:
        g = grid_geometry(width, height)
        grid = (g[0], g[2], g[4], g[5])
    p = InitParams(float(grid[0]), float(grid[1]), float(grid[2]), float(grid[3]), int(window), float(nnratio),
                   int(bool(check_orientation)))
    k1, d1, pv = _table(kps1, KEYPOINT_DTYPE), _desc(desc1), _table(prev_xy, np.float32, 2)
    k2, d2 = _table(kps2, KEYPOINT_DTYPE), _desc(desc2)
    n1, n2 = len(k1), len(k2)
    _same_len(n1, desc1=d1, prev_xy=pv)
    _same_len(n2, desc2=d2)
    c1, c2 = max(n1, 1), max(n2, 1)
    (bk1, bd1, bpv, bk2, bd2), cnt = _to_device(k1, d1, pv, k2, d2, counts=(n1, n2))
    co, ci, m = DeviceBuffer(4 * 3073), DeviceBuffer(4 * c2), DeviceBuffer(4 * c1)
    assign_grid_batch(bk2.ptr, cnt.ptr + 4, c2, 1, GridParams(*[float(v) for v in grid]), co.ptr, ci.ptr)
    search_for_initialization_batch(1, p, bk1.ptr, bd1.ptr, cnt.ptr, c1, bpv.ptr, bk2.ptr, bd2.ptr, cnt.ptr + 4, c2,
                                    co.ptr, ci.ptr, m.ptr, cnt.ptr + 8)
    _sync()
    nm = int(cnt.download(np.zeros(4, np.int32))[2])
    return nm, m.download(np.zeros(c1, np.int32))[:n1], bpv.download(np.zeros((c1, 2), np.float32))[:n1]


def line_search_init_batch(d_desc1, d_n1, cap1, d_desc2, d_n2, cap2, n_pairs, d_scratch, d_pairs, d_npairs, d_mad=0,
                           stream=None):
    """LineMatcher::SerachForInitialize + Frame::lineDescriptorMAD over device pair tables."""
    _call("plvi_line_search_init_batch", d_desc1, d_n1, cap1, d_desc2, d_n2, cap2, n_pairs, d_scratch, d_pairs,
          d_npairs, d_mad, stream or None)


def line_search_triangulation_batch(d_desc1, d_n1, cap1, d_desc2, d_n2, cap2, n_pairs, d_has_line1, d_has_line2,
                                    d_scratch, d_pairs, d_npairs, d_mad=0, stream=None):
    """LineMatcher::SearchForTriangulation (src/LineMatcher.cpp:142-171) over device pair tables."""
    _call("plvi_line_search_triangulation_batch", d_desc1, d_n1, cap1, d_desc2, d_n2, cap2, n_pairs, d_has_line1,
          d_has_line2, d_scratch, d_pairs, d_npairs, d_mad, stream or None)


def search_for_triangulation_batch(n_pairs, d_pairs, cap1, cap2, node_cap, kf1, kf2, d_matches12, d_nmatches,
                                   stream=None):
    """ORBmatcher::SearchForTriangulation over device pair tables (plvi_search_for_triangulation_batch).
    d_pairs: TriangulationPair [n_pairs]; kf1 / kf2: the nine device pointers of one side in header order
    (kps, desc, n, node, off, nnodes, idx, has_point, uright)."""
    if len(kf1) != 9 or len(kf2) != 9:
        raise ValueError("kf1 / kf2: nine device pointers each")
    _call("plvi_search_for_triangulation_batch", n_pairs, d_pairs, cap1, cap2, node_cap, *kf1, *kf2, d_matches12,
          d_nmatches, stream or None)


def search_by_bow_kf_batch(n_pairs, nnratio, check_orientation, cap1, cap2, node_cap, kf1, kf2, d_matches12,
                           d_nmatches, stream=None):
    """ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*) over device pair tables (plvi_search_by_bow_kf_batch).
    kf1 / kf2: the eight device pointers of one side in header order (desc, angle, live, n, node, off, nnodes,
    idx)."""
    if len(kf1) != 8 or len(kf2) != 8:
        raise ValueError("kf1 / kf2: eight device pointers each")
    _call("plvi_search_by_bow_kf_batch", n_pairs, float(nnratio), int(check_orientation), cap1, cap2, node_cap, *kf1,
          *kf2, d_matches12, d_nmatches, stream or None)


def search_sim3_projection_batch(n_pairs, params, kf, kp_cap, points, pt_cap, d_match, d_nmatches, stream=None):
    """Both ORBmatcher::SearchByProjection(pKF, Scw, ...) overloads over device tables
    (plvi_search_sim3_projection_batch).  params: Sim3ProjParams; kf: the six device pointers of the keyframe
    side in header order (kps, desc, n, matched (0 = none), cell_off, cell_idx); points: the seven of the point
    side (flags, x3dc, dist, dot, level, desc, n)."""
    if len(kf) != 6 or len(points) != 7:
        raise ValueError("kf: six device pointers, points: seven")
    kps, desc, n, matched, cell_off, cell_idx = kf
    _call("plvi_search_sim3_projection_batch", n_pairs, params, kps, desc, n, kp_cap, matched or None, cell_off,
          cell_idx, *points, pt_cap, d_match, d_nmatches, stream or None)


def fuse_points_batch(n_pairs, params, kf, kp_cap, points, pt_cap, d_fuse_idx, d_fuse_dist, d_nfused, stream=None):
    """Both ORBmatcher::Fuse overloads over device tables (plvi_fuse_points_batch).  params: FuseParams (mode set by
    the caller); kf: the six device pointers of the keyframe side in header order (kps, desc, n, uright (0 =
    monocular), cell_off, cell_idx); points: the seven of the point side (flags, x3dc, dist, dot, level, desc, n).
    nfused is written by the call."""
    if len(kf) != 6 or len(points) != 7:
        raise ValueError("kf: six device pointers, points: seven")
    kps, desc, n, uright, cell_off, cell_idx = kf
    _call("plvi_fuse_points_batch", n_pairs, params, kps, desc, n, kp_cap, uright or None, cell_off, cell_idx,
          *points, pt_cap, d_fuse_idx, d_fuse_dist, d_nfused, stream or None)


def fuse_lines_batch(n_pairs, params, kf, kl_cap, lines, ml_cap, d_fuse_idx, d_fuse_dist, d_nfused, stream=None):
    """LineMatcher::Fuse over device tables (plvi_fuse_lines_batch).  params: FuseLineParams; kf: the three device
    pointers of the keyframe side (keylines, desc, n); lines: the eight of the MapLine side (flags, spc, epc, dist,
    dot, level, desc, n)."""
    if len(kf) != 3 or len(lines) != 8:
        raise ValueError("kf: three device pointers, lines: eight")
    _call("plvi_fuse_lines_batch", n_pairs, params, *kf, kl_cap, *lines, ml_cap, d_fuse_idx, d_fuse_dist, d_nfused,
          stream or None)


def distinctive_descriptors_batch(n_feat, d_pool, pool_rows, d_obs_off, d_obs_row, max_obs, d_best_pos, d_best_median,
                                  d_out_desc=0, stream=None):
    """MapPoint / MapLine::ComputeDistinctiveDescriptors over device tables (plvi_distinctive_descriptors_batch).
    d_pool: pool_rows descriptor rows of 32 bytes (e.g. the keyframes' device tables back to back); d_obs_off
    [n_feat + 1], d_obs_row: the CSR observation lists (pool rows in the caller's order; a row outside the pool is
    ignored); max_obs: the clamp of every list length (<= DISTINCTIVE_MAX_OBS).  Outputs d_best_pos, d_best_median
    [n_feat] (-1 / -1 where no entry remains) and d_out_desc [n_feat][32] (0 = not wanted; a row is written only
    where best_pos >= 0).  Asynchronous on `stream`."""
    _call("plvi_distinctive_descriptors_batch", n_feat, d_pool or None, pool_rows, d_obs_off, d_obs_row or None,
          max_obs, d_best_pos, d_best_median, d_out_desc or None, stream or None)


def distinctive_descriptors(pool, obs_off, obs_row, out_desc=None):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:330-404) / MapLine::ComputeDistinctiveDescriptors
    (src/MapLine.cc:264-331) from host arrays.  pool: n x 32 uint8 descriptor rows; obs_off [n_feat + 1]
    (non-decreasing), obs_row: per feature the pool rows of its observations in the reference's list order (a row
    outside [0, n) is ignored, e.g. -1 for an absent leftIndex / rightIndex).  Returns (count, best_pos, best_median,
    out_desc): per feature the position inside its list of the first row with the least median distance (ignored
    entries counted; -1 when none remains), that median, and the row itself -- rows of `out_desc` (n_feat x 32,
    default zeros) with best_pos = -1 are left as passed in; count = features with best_pos >= 0."""
    pool, off, rows = _desc(pool), _table(obs_off, np.int32), _table(obs_row, np.int32)
    n_feat = len(off) - 1
    if n_feat < 0 or (n_feat > 0 and len(rows) < int(off[-1])):
        raise ValueError("obs_off: n_feat + 1 offsets into obs_row")
    res = np.zeros((max(n_feat, 0), 32), np.uint8) if out_desc is None else out_desc
    if res.dtype != np.uint8 or res.shape != (n_feat, 32) or not res.flags.c_contiguous:
        raise ValueError("out_desc: a C-contiguous n_feat x 32 uint8 array")
    bp, bm = _out(n_feat, -7), _out(n_feat, -7)
    n = _call("plvi_distinctive_descriptors", pool, len(pool), off, rows, n_feat, bp, bm, res)
    return n, bp[:n_feat], bm[:n_feat], res


def line_search_init(desc1, desc2):
    """One pair from host arrays: returns (LineMatches as an n x 2 int array
    (query, train), (nn_mad, nn12_mad))."""
    return _line_pairs_one(line_search_init_batch, desc1, desc2)[1:]


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
    kl, dl = _table(kpsL, KEYPOINT_DTYPE), _desc(descL)
    kr, dr = _table(kpsR, KEYPOINT_DTYPE), _desc(descR)
    _same_len(len(kl), descL=dl)
    _same_len(len(kr), descR=dr)
    bl, off, w, h = pack_pyramid(pyrL)
    br, off2, w2, h2 = pack_pyramid(pyrR)
    if not (np.array_equal(off, off2) and np.array_equal(w, w2) and np.array_equal(h, h2)):
        raise ValueError("left and right pyramids differ in geometry")
    sc, inv = _table(scale_factors, np.float32), _table(inv_scale_factors, np.float32)
    n = len(kl)
    ur, dp = _out(n, -1, np.float32), _out(n, -1, np.float32)
    k = _call("plvi_stereo_match", kl, dl, n, kr, dr, len(kr), len(pyrL), sc, inv, bl, br, off, w, h, float(mb),
              float(mbf), ur, dp)
    return k, ur[:n], dp[:n]


def stereo_match_batch(left, right, n_frames, mb, mbf, d_uright, d_depth, d_nstereo, d_err, stream=None):
    """plvi_stereo_match_batch on two ORBextractor handles (device outputs, asynchronous)."""
    _call("plvi_stereo_match_batch", left._h, right._h, n_frames, float(mb), float(mbf), d_uright, d_depth, d_nstereo,
          d_err, stream or None)


def ComputeStereoMatches_Lines(klL, descL, klR, descR, klUn, width, height, mbf, range_hint=1):
    """Frame::ComputeStereoMatches_Lines (src/Frame.cc:1408-1492) for one pair: mvKeys_Line, mvKeysRight_Line,
    mvKeysUn_Line (KEYLINE_DTYPE), LBD descriptors.  Returns (nstereo, matches_12, mvDisparity_l (n x 2),
    mvDepth_l (n x 2), mvle_l (n x 3))."""
    a, dl = _table(klL, KEYLINE_DTYPE), _desc(descL)
    b, dr = _table(klR, KEYLINE_DTYPE), _desc(descR)
    u = a if klUn is None else _table(klUn, KEYLINE_DTYPE)
    n = len(a)
    _same_len(n, descL=dl, klUn=u)
    _same_len(len(b), descR=dr)
    m, le = _out(n, -1), _out(n, 0, np.float64, 3)
    disp, dep = _out(n, -1, np.float32, 2), _out(n, -1, np.float32, 2)
    k = _call("plvi_stereo_lines", a, dl, n, b, dr, len(b), u, int(width), int(height), float(mbf), int(range_hint),
              m, disp, dep, le)
    return k, m[:n], disp[:n], dep[:n], le[:n]


def stereo_lines_scratch_bytes(n_frames, capL, capR, idx_cap):
    return load().plvi_stereo_lines_scratch_bytes(n_frames, capL, capR, idx_cap)


def stereo_lines_batch(n_frames, d_klL, d_descL, d_nL, capL, d_klR, d_descR, d_nR, capR, d_klUn, width, height,
                       mbf, range_hint, idx_cap, d_scratch, scratch_bytes, d_m12, d_disp, d_depth, d_le, d_nstereo,
                       d_err, stream=None):
    """plvi_stereo_lines_batch on device keyline tables (asynchronous)."""
    _call("plvi_stereo_lines_batch", n_frames, d_klL, d_descL, d_nL, capL, d_klR, d_descR, d_nR, capR, d_klUn or None,
          width, height, float(mbf), range_hint, idx_cap, d_scratch, scratch_bytes, d_m12, d_disp, d_depth, d_le,
          d_nstereo, d_err, stream or None)


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
    return _status("plvi_local_map_batch", n_frames, kf, mp, ml, frames, out, d_scratch or None, scratch_bytes,
                   stream or None)


_LM_ROWS = {"pos": (np.float32, 3), "sep": (np.float64, 6), "normal": (np.float32, 3), "dist": (np.float32, 2),
            "desc": (np.uint8, 32)}


def _pool_structs(pools, ptr):
    """LocalMapPool of the MapPoint and the MapLine pool (None where there is none); ptr as in _structs."""
    res = []
    for g, p in zip(("mp", "ml"), pools):
        s = None if p is None else LocalMapPool(len(p["bad"]))
        for k in p or ():
            setattr(s, k, ptr(g, k))
        res.append(s)
    return res


def _named_tables(kf, pools):
    """{(group, name): array} of a keyframe dict and the two pools."""
    t = {("kf", k): a for k, a in kf.items()}
    for g, p in zip(("mp", "ml"), pools):
        if p is not None:
            t.update({(g, k): a for k, a in p.items()})
    return t


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
        self.kf = {"bad": _table(kf["bad"], np.uint8)}
        for k in ("order", "covis", "child_off", "child", "parent", "prev_kf", "mp", "nmp", "ml", "nml"):
            if kf.get(k) is not None:
                self.kf[k] = _table(kf[k], np.int32)
        self.kf_cap = len(self.kf["bad"])
        self.kp_cap = self.kf["mp"].shape[1] if "mp" in self.kf and self.kf["mp"].ndim == 2 else 0
        self.kl_cap = self.kf["ml"].shape[1] if "ml" in self.kf and self.kf["ml"].ndim == 2 else 0
        self.pools = [self._pool(points), None if lines is None else self._pool(lines)]
        self.dev = None

    @staticmethod
    def _pool(p):
        q = {"bad": _table(p["bad"], np.uint8), "obs_off": _table(p["obs_off"], np.int32),
             "obs_kf": _table(p["obs_kf"], np.int32)}
        for k, (dt, w) in _LM_ROWS.items():
            if p.get(k) is not None:
                q[k] = np.ascontiguousarray(p[k], dt).reshape(len(q["bad"]), w)
        return q

    def _structs(self, ptr):
        """The keyframe and pool structs; ptr(group, name) -> the address of that table or None."""
        kf = LocalMapKeyframes(self.kf_cap, len(self.kf.get("order", ())), self.kp_cap, self.kl_cap)
        for k in self.kf:
            setattr(kf, k, ptr("kf", k))
        return (kf, *_pool_structs(self.pools, ptr))

    def _tables(self):
        return _named_tables(self.kf, self.pools)

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
        rc = _status("plvi_local_map", kf, mp, ml, fr, out)
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
            tabs = self._tables()
            self.dev = dict(zip(tabs, _to_device(*tabs.values())[0]))
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
            _sync()
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
        _call("plvi_covis_create", kf_cap, conn_cap, device, ctypes.byref(h))
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
        self.kf = {k: _table(keyframes[k], dt) for k, dt in _COVIS_KF.items() if keyframes.get(k) is not None}
        pool = lambda p: None if p is None else {  # noqa: E731
            "bad": _table(p["bad"], np.uint8), "obs_off": _table(p["obs_off"], np.int32),
            "obs_kf": _table(p["obs_kf"], np.int32)}
        self.pools = [pool(points), pool(lines)]
        self.dev = {}
        for key, a in self._tables().items():
            self.put(key[0], key[1], a)
        return self

    def _tables(self):
        return _named_tables(self.kf, self.pools)

    def put(self, group, name, a):
        """Replace one resident table (group "kf", "mp" or "ml")."""
        a = _table(a, _COVIS_KF[name] if group == "kf" else (np.uint8 if name == "bad" else np.int32))
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
        return (kf, *_pool_structs(self.pools, ptr))

    def update_batch(self, q_slots, fill=-7, stream=None, run=True):
        """plvi_covis_update_batch of the keyframes q_slots, in that order.  Returns a dict of the per-query
        outputs (sentinel-filled with `fill` where nothing was written), "past" (the cell after the last query of
        each output: `fill` unless something wrote past the batch) and "rc".  run=False returns (step(stream),
        fetch()) instead, for graph capture."""
        q = _table(q_slots, np.int32)
        B = len(q)
        kf, mp, ml = self._structs(lambda g, k: self.dev[(g, k)].ptr)
        res = {k: np.full(B + 1, fill, np.int32) for k in _COVIS_OUT}   # one cell more than is written
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        out = CovisOutputs(*[obuf[k].ptr for k in _COVIS_OUT])
        sb = covis_scratch_bytes(B, self.kf_cap)
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_covis_update_batch", self.h, B, q, kf, mp, ml, out, scratch.ptr, sb, s or None)

        def fetch(rc=0):
            _sync()
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
        rc = _status("plvi_covis_update", self.h, int(slot), kf, mp, ml, out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_covis_update")
        r = {k: int(a[0]) for k, a in res.items()}
        r["rc"] = rc
        return r

    def _slots_call(self, name, slots, stream):
        s = _table(slots, np.int32)
        cov = self.dev.get(("kf", "covis"))
        return _status(name, self.h, len(s), s, self.dev[("kf", "bad")].ptr, self.dev[("kf", "order")].ptr,
                       len(self.kf["order"]), cov.ptr if cov else None, stream or None)

    def erase(self, slots, stream=None):
        """The connection part of SetBadFlag for `slots` (plvi_covis_erase_batch); returns the status."""
        return self._slots_call("plvi_covis_erase_batch", slots, stream)

    def resort(self, slots, stream=None):
        """UpdateBestCovisibles of `slots` (plvi_covis_resort_batch); returns the status."""
        return self._slots_call("plvi_covis_resort_batch", slots, stream)

    def _pairs(self, name, a, b):
        a, b = _table(a, np.int32), _table(b, np.int32)
        assert a.shape == b.shape
        (da, db), _ = _to_device(a, b)
        do = DeviceBuffer(a.nbytes)
        _call(name, self.h, len(a), da.ptr, db.ptr, do.ptr, None)
        _sync()
        return do.download(np.empty_like(a))

    def by_weight(self, slots, weights):
        """len(GetCovisiblesByWeight(w)) per (slot, w)."""
        return self._pairs("plvi_covis_by_weight_batch", slots, weights)

    def weight(self, a, b):
        """a->GetWeight(b) per pair of slots."""
        return self._pairs("plvi_covis_weight_batch", a, b)

    def rows(self):
        """(ord_kf, ord_w, ord_n) device addresses of the ordered tables [kf_cap][conn_cap] and their counts."""
        p = [ctypes.c_void_p() for _ in range(3)]
        c = ctypes.c_int()
        _call("plvi_covis_rows", self.h, *[ctypes.byref(x) for x in p], ctypes.byref(c))
        return tuple(x.value for x in p)

    def map_rows(self):
        """(map_kf, map_w, map_n) device addresses of the weight-map tables [kf_cap][conn_cap], rows unsorted, and
        their counts."""
        p = [ctypes.c_void_p() for _ in range(3)]
        c = ctypes.c_int()
        _call("plvi_covis_map_rows", self.h, *[ctypes.byref(x) for x in p], ctypes.byref(c))
        return tuple(x.value for x in p)

    def download(self, slot, fill=-7):
        """One slot's state: dict(map_kf, map_w (ascending slot), ord_kf, ord_w (as stored), err).  The arrays are
        conn_cap + 1 long and sentinel-filled past their counts n_map / n_ord."""
        C = self.conn_cap
        t = {k: np.full(C + 1, fill, np.int32) for k in ("map_kf", "map_w", "ord_kf", "ord_w")}
        n = [ctypes.c_int() for _ in range(3)]
        _call("plvi_covis_download", self.h, int(slot), t["map_kf"], t["map_w"], ctypes.byref(n[0]), t["ord_kf"],
              t["ord_w"], ctypes.byref(n[1]), ctypes.byref(n[2]))
        t.update(n_map=n[0].value, n_ord=n[1].value, err=n[2].value)
        return t


CULL_MAX_CHANGED = 128  # PLVI_CULL_MAX_CHANGED: keyframes a walk's overlay holds
CULL_SPEC = 101         # PLVI_CULL_SPEC: candidates whose counts are taken ahead of the walk
CULL_STOP_END, CULL_STOP_BREAK_ABORT, CULL_STOP_BREAK_100, CULL_STOP_NEEDS_NORM = 0, 1, 2, 3
(CULL_NOT_VISITED, CULL_SKIP_INIT, CULL_SKIP_BAD, CULL_KEEP, CULL_KEEP_FEW_KF, CULL_KEEP_RECENT, CULL_KEEP_NO_CHAIN,
 CULL_KEEP_TIME, CULL_KEEP_NORM, CULL_CULLED, CULL_CULLED_TIME, CULL_CULLED_NORM, CULL_NEEDS_NORM) = range(13)
CULL_DEFERRED = 0x80
CULL_KIND_POINTS, CULL_KIND_LINES, CULL_KIND_RELINKED, CULL_KIND_DEFERRED = 1, 2, 4, 8
CULL_ERR_OUT, CULL_ERR_CHANGED, CULL_ERR_PRE, CULL_ERR_QUERY = 1, 2, 4, 8

_CULL_KF = {"bad": np.uint8, "init_kf": np.uint8, "not_erase": np.uint8, "mp": np.int32, "nmp": np.int32,
            "ml": np.int32, "nml": np.int32, "kp_info": np.uint8, "kl_info": np.uint8, "cand": np.int32,
            "n_cand": np.int32, "kf_id": np.uint32, "timestamp": np.float64, "prev_kf": np.int32, "next_kf": np.int32}
_CULL_POOL = {"bad": np.uint8, "obs_off": np.int32, "obs_kf": np.int32, "obs_idx": np.int32, "nobs": np.int32}
_CULL_Q = ("q_slot", "abort_ba", "n_kf_in_map", "imu_init", "inertial_ba2")
_CULL_Q_OUT = ("n_visited", "stop", "n_kf_in_map", "err", "n_changed")
_CULL_CAND_OUT = {"outcome": np.uint8, "n_mps": np.int32, "n_mls": np.int32, "n_redundant": np.int32}
_CULL_CH_OUT = ("changed_slot", "changed_kind")


class CullKeyframes(ctypes.Structure):
    """plvi_cull_keyframes (include/plvi_frontend.h); pointers as integers, 0 / None = NULL."""
    _fields_ = [("kf_cap", _LM_I), ("kp_cap", _LM_I), ("kl_cap", _LM_I), ("cand_stride", _LM_I)] + \
               [(k, _LM_V) for k in _CULL_KF]


class CullFeatures(ctypes.Structure):
    """plvi_cull_features: what the walk reads of a pool besides plvi_local_map_pool."""
    _fields_ = [("obs_idx", _LM_V), ("nobs", _LM_V)]


class CullParams(ctypes.Structure):
    """plvi_cull_params."""
    _fields_ = [("redundant_th", ctypes.c_float), ("monocular", _LM_I), ("inertial", _LM_I), ("slam_mode", _LM_I)]


class CullQueries(ctypes.Structure):
    """plvi_cull_queries: per-query arrays."""
    _fields_ = [(k, _LM_V) for k in _CULL_Q + ("start", "verdict")] + \
               [("pre_cap", _LM_I), ("pre_n", _LM_V), ("pre_slot", _LM_V), ("pre_kind", _LM_V)]


class CullOutputs(ctypes.Structure):
    """plvi_cull_outputs."""
    _fields_ = [("out_cap", _LM_I), ("changed_cap", _LM_I)] + \
               [(k, _LM_V) for k in ("n_visited", "stop", "n_kf_in_map", "err", "outcome", "n_mps", "n_mls",
                                     "n_redundant", "n_changed", "changed_slot", "changed_kind")]


class KeyFrameCulling:
    """LocalMapping::KeyFrameCulling() / KeyFrameCullingWithLines() (src/LocalMapping.cc:1566-1964) over resident
    tables (plvi_keyframe_culling[_batch]): the redundancy walk over the covisibles of a current keyframe.

    ``keyframes``: a dict of numpy arrays named as the fields of plvi_cull_keyframes -- bad, mp, nmp, kp_info, cand
    [kf_cap][cand_stride], n_cand, and optionally init_kf, not_erase, ml / nml / kl_info (ml selects the lines
    function) and, for inertial, kf_id, timestamp, prev_kf, next_kf.  ``points`` / ``lines``: dicts with bad,
    obs_off, obs_kf, obs_idx and optionally nobs.  ``rows`` = (d_ord_kf, d_ord_n, conn_cap), the device addresses
    of Covisibility.rows(), replaces cand / n_cand in the batch form: the graph's rows are walked in place.

    ``cull_batch`` runs on device copies (``self.dev``); ``cull`` runs one query through the host form.  Both return
    a dict: n_visited, stop, n_kf_in_map, err, n_changed per query, outcome / n_mps / n_mls / n_redundant [q][out_cap]
    by candidate position, changed_slot / changed_kind [q][changed_cap], sentinel-filled where nothing was written.
    A walk that stopped for cv::norm is resumed by passing that dict as ``prev`` with ``verdict``."""

    def __init__(self, keyframes, points, lines=None, redundant_th=0.9, monocular=True, inertial=False, slam_mode=0,
                 rows=None):
        self._lib = load()
        self.kf = {k: _table(keyframes[k], dt) for k, dt in _CULL_KF.items() if keyframes.get(k) is not None}
        pool = lambda p: None if p is None else {  # noqa: E731
            k: _table(p[k], dt) for k, dt in _CULL_POOL.items() if p.get(k) is not None}
        self.pools = [pool(points), pool(lines)]
        self.kf_cap = len(self.kf["bad"])
        self.params = CullParams(redundant_th, int(monocular), int(inertial), int(slam_mode))
        self.rows = rows
        self.dev = None

    def _structs(self, ptr, rows=None):
        shape = lambda k: self.kf[k].shape[1] if k in self.kf and self.kf[k].ndim == 2 else 0  # noqa: E731
        kf = CullKeyframes(self.kf_cap, shape("mp"), shape("ml"), rows[2] if rows else shape("cand"))
        for k in self.kf:
            setattr(kf, k, ptr("kf", k))
        if rows:
            kf.cand, kf.n_cand = rows[0], rows[1]
        res = [kf]
        for g, p in zip(("mp", "ml"), self.pools):
            if p is None:
                res += [None, None]
                continue
            s, f = LocalMapPool(len(p["bad"])), CullFeatures()
            for k in p:
                setattr(f if k in ("obs_idx", "nobs") else s, k, ptr(g, k))
            res += [s, f]
        return res

    def upload(self):
        if self.dev is None:
            tabs = _named_tables(self.kf, self.pools)
            self.dev = dict(zip(tabs, _to_device(*tabs.values())[0]))
        return self.dev

    @staticmethod
    def _host(B, q_slot, abort_ba, n_kf_in_map, imu_init, inertial_ba2, start, verdict, prev, out_cap, changed_cap,
              fill):
        """The per-query inputs and the pre-filled outputs as host arrays."""
        per = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (B,)))  # noqa: E731
        qin = dict(zip(_CULL_Q, map(per, (q_slot, abort_ba, n_kf_in_map, imu_init, inertial_ba2))))
        res = {k: np.full(B + 1, fill, np.int32) for k in _CULL_Q_OUT}  # one cell more than is written
        for k, dt in _CULL_CAND_OUT.items():
            res[k] = np.full((B + 1, max(out_cap, 1)), fill & 0x7f if dt == np.uint8 else fill, dt)
        for k in _CULL_CH_OUT:
            res[k] = np.full((B + 1, max(changed_cap, 1)), fill, np.int32)
        if start is not None or verdict is not None or prev is not None:
            qin["start"] = per(0 if start is None else start)
            qin["verdict"] = per(-1 if verdict is None else verdict)
            qin["pre_n"] = per(0)
            qin["pre_slot"] = np.zeros((B, max(changed_cap, 1)), np.int32)
            qin["pre_kind"] = np.zeros((B, max(changed_cap, 1)), np.int32)
            if prev is not None:  # the earlier call's outputs stay where this call does not write
                for k in _CULL_CAND_OUT:
                    res[k][:B] = prev[k]
                qin["pre_n"] = per(prev["n_changed"])
                qin["pre_slot"][:] = prev["changed_slot"]
                qin["pre_kind"][:] = prev["changed_kind"]
                if start is None:
                    qin["start"] = per(np.maximum(prev["n_visited"] - 1, 0))
        return qin, res

    def cull_batch(self, q_slot, abort_ba=0, n_kf_in_map=0, imu_init=0, inertial_ba2=0, start=None, verdict=None,
                   prev=None, out_cap=None, changed_cap=None, fill=-7, stream=None, run=True):
        """plvi_keyframe_culling_batch of the current keyframes q_slot (the other per-query arguments broadcast).
        Returns the dict described above plus "past" (the row after the last query of every output: `fill`
        unless something wrote past the batch) and "rc".  run=False returns (step(stream), fetch()) for capture."""
        dev = self.upload()
        structs = self._structs(lambda g, k: dev[(g, k)].ptr, self.rows)
        B = len(np.atleast_1d(q_slot))
        out_cap = (self.rows[2] if self.rows else structs[0].cand_stride) if out_cap is None else out_cap
        changed_cap = CULL_MAX_CHANGED if changed_cap is None else changed_cap
        qin, res = self._host(B, np.atleast_1d(q_slot), abort_ba, n_kf_in_map, imu_init, inertial_ba2, start, verdict,
                              prev, out_cap, changed_cap, fill)
        qbuf = dict(zip(qin, _to_device(*qin.values())[0]))
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        qs = CullQueries(pre_cap=max(changed_cap, 1) if "pre_n" in qin else 0)
        for k, b in qbuf.items():
            setattr(qs, k, b.ptr)
        out = CullOutputs(out_cap, changed_cap)
        for k, b in obuf.items():
            setattr(out, k, b.ptr)

        sb = load().plvi_keyframe_culling_scratch_bytes(B)
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_keyframe_culling_batch", B, *structs, self.params, qs, out, scratch.ptr, sb,
                           s or None)

        def fetch(rc=0):
            _sync()
            full = {k: obuf[k].download(a) for k, a in res.items()}
            r = {k: a[:B] for k, a in full.items()}
            r.update(rc=rc, past={k: a[B].tolist() for k, a in full.items()}, keep=(qbuf, obuf, scratch))
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def cull(self, q_slot, abort_ba=0, n_kf_in_map=0, imu_init=0, inertial_ba2=0, start=None, verdict=None,
             prev=None, out_cap=None, changed_cap=None, fill=-7):
        """One query through the host form (plvi_keyframe_culling); the same dict with one query, and "rc"
        (PLVI_E_CAPACITY with an err bit set; any other refusal raises)."""
        tabs = _named_tables(self.kf, self.pools)
        structs = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        out_cap = structs[0].cand_stride if out_cap is None else out_cap
        changed_cap = CULL_MAX_CHANGED if changed_cap is None else changed_cap
        qin, res = self._host(1, [q_slot], abort_ba, n_kf_in_map, imu_init, inertial_ba2, start, verdict, prev,
                              out_cap, changed_cap, fill)
        qs = CullQueries(pre_cap=max(changed_cap, 1) if "pre_n" in qin else 0)
        for k, a in qin.items():
            setattr(qs, k, a.ctypes.data)
        out = CullOutputs(out_cap, changed_cap)
        for k, a in res.items():
            setattr(out, k, a.ctypes.data)
        rc = _status("plvi_keyframe_culling", *structs, self.params, qs, out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_keyframe_culling")
        r = {k: a[:1] for k, a in res.items()}
        r.update(rc=rc, past={k: a[1].tolist() for k, a in res.items()})
        return r


BA_LDS_KF = 2048              # PLVI_BA_LDS_KF: largest kf_cap whose per-slot tables are kept in LDS
BA_MAX_OPT = 64               # PLVI_BA_MAX_OPT
BA_MAX_FIXED_INERTIAL = 200   # PLVI_BA_MAX_FIXED_INERTIAL
BA_POINTS, BA_LINES, BA_INERTIAL = range(3)
BA_EDGE_MONO, BA_EDGE_STEREO, BA_EDGE_LINE = range(3)
BA_ERR_LOCAL_KF, BA_ERR_FIXED_KF, BA_ERR_FEAT, BA_ERR_EDGE, BA_ERR_UNDEFINED, BA_ERR_QUERY = 1, 2, 4, 8, 16, 32

_BA_POOL = {"bad": np.uint8, "obs_off": np.int32, "obs_kf": np.int32, "obs_idx": np.int32, "map_id": np.int32}
_BA_Q_OUT = ("n_local_kf", "n_fixed_kf", "num_fixed", "init_in_local", "non_fixed", "n_local_feat", "n_mono",
             "n_stereo", "n_line", "err")
_BA_LISTS = {"local_kf": "lkf_cap", "fixed_kf": "fkf_cap", "local_feat": "feat_cap", "edge_feat": "edge_cap",
             "edge_kf": "edge_cap", "edge_idx": "edge_cap", "edge_cam": "edge_cap", "edge_kind": "edge_cap"}


class BAFeatures(ctypes.Structure):
    """plvi_ba_features."""
    _fields_ = [("obs_idx", _LM_V), ("map_id", _LM_V)]


class BAParams(ctypes.Structure):
    """plvi_ba_params."""
    _fields_ = [("mode", _LM_I), ("max_opt", _LM_I)]


class BAQueries(ctypes.Structure):
    """plvi_ba_queries."""
    _fields_ = [("q_slot", _LM_V), ("n_kf_in_map", _LM_V)]


class BAOutputs(ctypes.Structure):
    """plvi_ba_outputs."""
    _fields_ = [(k, _LM_I) for k in ("lkf_cap", "fkf_cap", "feat_cap", "edge_cap")] + \
               [(k, _LM_V) for k in ("local_kf", "n_local_kf", "fixed_kf", "n_fixed_kf", "num_fixed", "init_in_local",
                                     "non_fixed", "local_feat", "n_local_feat", "edge_feat", "edge_kf", "edge_idx",
                                     "edge_cam", "edge_kind", "n_mono", "n_stereo", "n_line", "err")]


class LocalBAWindow:
    """The set-up of Optimizer::LocalBundleAdjustment / LocalBundleAdjustmentOnlyLines[Angle|WithAngle] /
    LocalInertialBA (src/Optimizer.cc:4851-4960, :6181-6233, :9185-9307 and their edge loops) over resident tables
    (plvi_ba_window[_batch]): local keyframes, local features, fixed cameras and the edge list of a current keyframe.

    ``keyframes``: a dict of numpy arrays named as the fields of plvi_cull_keyframes -- bad, mp / nmp / kp_info
    (POINTS, INERTIAL) or ml / nml (LINES), cand / n_cand (visual modes), kf_id (POINTS), prev_kf (INERTIAL) and
    optionally init_kf.  ``points`` / ``lines``: dicts with bad, obs_off, obs_kf, obs_idx and optionally map_id.
    ``kf_map_id`` [kf_cap] is GetMap() per slot, None = one map.  ``rows`` as in KeyFrameCulling.

    ``batch`` runs on device copies (``self.dev``), ``host`` runs one query through the host form.  Both return a
    dict: the per-query counts and flags, local_kf / fixed_kf / local_feat and the edge_* arrays [q][cap],
    sentinel-filled where nothing was written."""

    def __init__(self, keyframes, points=None, lines=None, mode=BA_POINTS, max_opt=10, kf_map_id=None, rows=None):
        self._lib = load()
        self.kf = {k: _table(keyframes[k], dt) for k, dt in _CULL_KF.items() if keyframes.get(k) is not None}
        if kf_map_id is not None:
            self.kf["map_id"] = _table(kf_map_id, np.int32)
        pool = lambda p: None if p is None else {  # noqa: E731
            k: _table(p[k], dt) for k, dt in _BA_POOL.items() if p.get(k) is not None}
        self.pools = [pool(points), pool(lines)]
        self.kf_cap = len(self.kf["bad"])
        self.mode = int(mode)
        self.params = BAParams(self.mode, int(max_opt))
        self.rows = rows
        self.dev = None

    def _pool(self):
        return self.pools[1 if self.mode == BA_LINES else 0]

    def _check_tables(self):
        """Every companion array has the length its table gives it: refused here, before the library reads them."""
        _same_len(self.kf_cap, **{"keyframes." + k: a for k, a in self.kf.items()})
        for g, p in zip(("points", "lines"), self.pools):
            if p is None:
                continue
            n = len(p["bad"])
            _same_len(n + 1, **{g + ".obs_off": p["obs_off"]})
            _same_len(n, **{g + ".map_id": p.get("map_id")})
            n_obs = int(p["obs_off"][n]) if n else 0
            if len(p["obs_kf"]) < n_obs:
                raise ValueError(f"{g}.obs_kf has {len(p['obs_kf'])} records, obs_off names {n_obs}")
            _same_len(len(p["obs_kf"]), **{g + ".obs_idx": p.get("obs_idx")})
        if self._pool() is None:
            raise ValueError("the mode's pool is missing")

    def _structs(self, ptr, rows=None):
        shape = lambda k: self.kf[k].shape[1] if k in self.kf and self.kf[k].ndim == 2 else 0  # noqa: E731
        kf = CullKeyframes(self.kf_cap, shape("mp"), shape("ml"), rows[2] if rows else shape("cand"))
        for k in self.kf:
            if k != "map_id":
                setattr(kf, k, ptr("kf", k))
        if rows:
            kf.cand, kf.n_cand = rows[0], rows[1]
        res = [kf, ptr("kf", "map_id") if "map_id" in self.kf else None]
        for g, p in zip(("mp", "ml"), self.pools):
            if p is None:
                res += [None, None]
                continue
            s, f = LocalMapPool(len(p["bad"])), BAFeatures()
            for k in p:
                setattr(f if k in ("obs_idx", "map_id") else s, k, ptr(g, k))
            res += [s, f]
        return res

    def upload(self):
        if self.dev is None:
            tabs = _named_tables(self.kf, self.pools)
            self.dev = dict(zip(tabs, _to_device(*tabs.values())[0]))
        return self.dev

    def _caps(self, stride, lkf_cap, fkf_cap, feat_cap, edge_cap):
        p = self._pool()
        d = (max(stride, self.params.max_opt) + 1, self.kf_cap + 2, len(p["bad"]), len(p["obs_kf"]))
        return {k: d[i] if v is None else v
                for i, (k, v) in enumerate(zip(("lkf_cap", "fkf_cap", "feat_cap", "edge_cap"),
                                               (lkf_cap, fkf_cap, feat_cap, edge_cap)))}

    @staticmethod
    def _host(B, q_slot, n_kf_in_map, caps, fill):
        per = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (B,)))  # noqa: E731
        qin = {"q_slot": per(q_slot), "n_kf_in_map": per(n_kf_in_map)}
        res = {k: np.full(B + 1, fill, np.int32) for k in _BA_Q_OUT}  # one row more than is written
        for k, c in _BA_LISTS.items():
            dt = np.uint8 if k == "edge_kind" else np.int32
            res[k] = np.full((B + 1, max(caps[c], 1)), fill & 0x7f if dt == np.uint8 else fill, dt)
        return qin, res

    def batch(self, q_slot, n_kf_in_map=0, lkf_cap=None, fkf_cap=None, feat_cap=None, edge_cap=None, fill=-7,
              stream=None, run=True):
        """plvi_ba_window_batch of the current keyframes q_slot.  Returns the dict described above plus "past" (the
        row after the last query of every output) and "rc".  run=False returns (step(stream), fetch()) for capture."""
        self._check_tables()
        dev = self.upload()
        structs = self._structs(lambda g, k: dev[(g, k)].ptr, self.rows)
        B = len(np.atleast_1d(q_slot))
        caps = self._caps(structs[0].cand_stride, lkf_cap, fkf_cap, feat_cap, edge_cap)
        qin, res = self._host(B, np.atleast_1d(q_slot), n_kf_in_map, caps, fill)
        qbuf = dict(zip(qin, _to_device(*qin.values())[0]))
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        qs = BAQueries(**{k: b.ptr for k, b in qbuf.items()})
        out = BAOutputs(**caps)
        for k, b in obuf.items():
            setattr(out, k, b.ptr)
        n = [0 if p is None else len(p["bad"]) for p in self.pools]
        sb = load().plvi_ba_window_scratch_bytes(B, self.kf_cap, n[0], n[1])
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_ba_window_batch", B, *structs, self.params, qs, out, scratch.ptr, sb, s or None)

        def fetch(rc=0):
            _sync()
            full = {k: obuf[k].download(a) for k, a in res.items()}
            r = {k: a[:B] for k, a in full.items()}
            r.update(rc=rc, past={k: a[B].tolist() for k, a in full.items()}, keep=(qbuf, obuf, scratch))
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def host(self, q_slot, n_kf_in_map=0, lkf_cap=None, fkf_cap=None, feat_cap=None, edge_cap=None, fill=-7):
        """One query through the host form (plvi_ba_window); the same dict with one query, and "rc"
        (PLVI_E_CAPACITY with an overflow bit set; any other refusal raises)."""
        self._check_tables()
        tabs = _named_tables(self.kf, self.pools)
        structs = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        caps = self._caps(structs[0].cand_stride, lkf_cap, fkf_cap, feat_cap, edge_cap)
        qin, res = self._host(1, [q_slot], n_kf_in_map, caps, fill)
        qs = BAQueries(**{k: a.ctypes.data for k, a in qin.items()})
        out = BAOutputs(**caps)
        for k, a in res.items():
            setattr(out, k, a.ctypes.data)
        rc = _status("plvi_ba_window", *structs, self.params, qs, out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_ba_window")
        r = {k: a[:1] for k, a in res.items()}
        r.update(rc=rc, past={k: a[1].tolist() for k, a in res.items()})
        return r


LOOP_COVISIBLES = 5   # PLVI_LOOP_COVISIBLES: nNumCovisibles
LOOP_BOW_WIN = 6      # PLVI_LOOP_BOW_WIN: longest BOW window
LOOP_WIN_MAX = 31     # PLVI_LOOP_WIN_MAX: longest LAST window, row length of win
LOOP_WIN_BOW, LOOP_WIN_PROJ, LOOP_WIN_LAST = range(3)
LOOP_ERR_PTS, LOOP_ERR_UNDEFINED, LOOP_ERR_QUERY = 1, 2, 4

_LOOP_KF = {"bad": np.uint8, "mp": np.int32, "nmp": np.int32, "cand": np.int32, "n_cand": np.int32}
_LOOP_ROWS = {k: _LM_ROWS[k] for k in ("pos", "normal", "dist", "desc")}
_LOOP_Q_OUT = ("n_win", "abort_at", "n_pts", "err")
_LOOP_MERGE_OUT = ("matched_mp", "matched_kf")


class LoopQueries(ctypes.Structure):
    """plvi_loop_queries."""
    _fields_ = [(k, _LM_V) for k in ("kind", "kf_slot", "cur_slot", "conn_off", "conn_slot")]


class LoopOutputs(ctypes.Structure):
    """plvi_loop_outputs."""
    _fields_ = [("pt_cap", _LM_I)] + \
               [(k, _LM_V) for k in ("win", "n_win", "abort_at", "pts", "pts_kf", "n_pts", "pos", "normal", "dist",
                                     "desc", "err")]


class LoopWindow:
    """The keyframe windows, the BoW merge and the point clouds of LoopClosing::NewDetectCommonRegions
    (src/LoopClosing.cc:797-858, :893-915, :1162-1199) over resident tables (plvi_loop_window[_batch],
    plvi_loop_bow_merge[_batch]).

    ``keyframes``: a dict of numpy arrays named as the fields of plvi_cull_keyframes -- bad, mp / nmp, cand / n_cand.
    ``points``: a dict with bad and optionally pos, normal, dist, desc (the rows a gather reads).  ``rows`` as in
    KeyFrameCulling: the graph's rows replace cand / n_cand in the batch forms.

    ``batch`` runs on device copies (``self.dev``), ``host`` runs one query through the host form.  Both return a
    dict: n_win, abort_at, n_pts, err per query, win [q][31], pts / pts_kf [q][pt_cap] and the gathered rows asked
    for by ``gather``, sentinel-filled where nothing was written.  ``connected`` is one sequence of slots per query
    (GetConnectedKeyFrames() of the current keyframe), None = no keyframe is connected.  ``merge_batch`` /
    ``merge_host`` take the BOW windows and the six SearchByBoW tables per query."""

    def __init__(self, keyframes, points, rows=None):
        self._lib = load()
        self.kf = {k: _table(keyframes[k], dt) for k, dt in _LOOP_KF.items() if keyframes.get(k) is not None}
        p = {"bad": _table(points["bad"], np.uint8)}
        for k, (dt, w) in _LOOP_ROWS.items():
            if points.get(k) is not None:
                p[k] = _table(points[k], dt, w)
        self.pools = [p, None]
        self.kf_cap = len(self.kf["bad"])
        self.rows = rows
        self.dev = None

    def _check_tables(self):
        """Every companion array has the length its table gives it: refused here, before the library reads them."""
        _same_len(self.kf_cap, **{"keyframes." + k: a for k, a in self.kf.items()})
        p = self.pools[0]
        _same_len(len(p["bad"]), **{"points." + k: a for k, a in p.items()})

    def _structs(self, ptr, rows=None):
        shape = lambda k: self.kf[k].shape[1] if k in self.kf and self.kf[k].ndim == 2 else 0  # noqa: E731
        kf = CullKeyframes(self.kf_cap, shape("mp"), 0, rows[2] if rows else shape("cand"))
        for k in self.kf:
            setattr(kf, k, ptr("kf", k))
        if rows:
            kf.cand, kf.n_cand = rows[0], rows[1]
        return kf, _pool_structs(self.pools, ptr)[0]

    def upload(self):
        if self.dev is None:
            tabs = _named_tables(self.kf, self.pools)
            self.dev = dict(zip(tabs, _to_device(*tabs.values())[0]))
        return self.dev

    def _pt_cap(self, pt_cap):
        return max(len(self.pools[0]["bad"]), 1) if pt_cap is None else pt_cap

    def _host(self, B, kind, kf_slot, cur_slot, connected, pt_cap, gather, owners, fill):
        """The per-query inputs and the pre-filled outputs as host arrays."""
        per = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (B,)))  # noqa: E731
        qin = {"kind": per(kind), "kf_slot": per(kf_slot)}
        if cur_slot is not None:
            qin["cur_slot"] = per(cur_slot)
        if connected is not None:
            if len(connected) != B:
                raise ValueError(f"connected has {len(connected)} rows, expected {B}")
            off = np.zeros(B + 1, np.int32)
            off[1:] = np.cumsum([len(c) for c in connected])
            qin["conn_off"] = off
            qin["conn_slot"] = np.array([s for c in connected for s in c], np.int32).reshape(-1)
        for k in gather:
            if k not in self.pools[0]:
                raise ValueError(f"gather of {k}: points has no such row")
        res = {k: np.full(B + 1, fill, np.int32) for k in _LOOP_Q_OUT}  # one row more than is written
        res["win"] = np.full((B + 1, LOOP_WIN_MAX), fill, np.int32)
        c = max(pt_cap, 1)
        for k in ("pts", "pts_kf") if owners else ("pts",):
            res[k] = np.full((B + 1, c), fill, np.int32)
        for k in gather:
            dt, w = _LOOP_ROWS[k]
            res[k] = np.full((B + 1, c, w), fill & 0x7f if dt == np.uint8 else fill, dt)
        return qin, res

    def batch(self, kind, kf_slot, cur_slot=None, connected=None, pt_cap=None, gather=(), owners=True, fill=-7,
              stream=None, run=True):
        """plvi_loop_window_batch of the queries (kind, kf_slot), which broadcast against each other.  Returns the
        dict described above plus "past" (the row after the last query of every output), "dev" (the device address
        of every output, for the calls that follow) and "rc".  run=False returns (step(stream), fetch())."""
        self._check_tables()
        B = np.broadcast(np.atleast_1d(kind), np.atleast_1d(kf_slot)).shape[0]
        pt_cap = self._pt_cap(pt_cap)
        qin, res = self._host(B, kind, kf_slot, cur_slot, connected, pt_cap, gather, owners, fill)
        dev = self.upload()
        structs = self._structs(lambda g, k: dev[(g, k)].ptr, self.rows)
        qbuf = dict(zip(qin, _to_device(*qin.values())[0]))
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        qs = LoopQueries(**{k: b.ptr for k, b in qbuf.items()})
        out = LoopOutputs(pt_cap, **{k: b.ptr for k, b in obuf.items()})
        sb = load().plvi_loop_window_scratch_bytes(B, len(self.pools[0]["bad"]))
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_loop_window_batch", B, *structs, qs, out, scratch.ptr, sb, s or None)

        def fetch(rc=0):
            _sync()
            full = {k: obuf[k].download(a) for k, a in res.items()}
            r = {k: a[:B] for k, a in full.items()}
            r.update(rc=rc, past={k: a[B].tolist() for k, a in full.items()}, keep=(qbuf, obuf, scratch),
                     dev={k: b.ptr for k, b in obuf.items()})
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def host(self, kind, kf_slot, cur_slot=None, connected=None, pt_cap=None, gather=(), owners=True, fill=-7):
        """One query through the host form (plvi_loop_window); the same dict with one query, and "rc"
        (PLVI_E_CAPACITY with PTS or QUERY set; any other refusal raises).  connected: the slots of this query."""
        self._check_tables()
        tabs = _named_tables(self.kf, self.pools)
        structs = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        pt_cap = self._pt_cap(pt_cap)
        qin, res = self._host(1, [kind], [kf_slot], None if cur_slot is None else [cur_slot],
                              None if connected is None else [connected], pt_cap, gather, owners, fill)
        qs = LoopQueries(**{k: a.ctypes.data for k, a in qin.items()})
        out = LoopOutputs(pt_cap, **{k: a.ctypes.data for k, a in res.items()})
        rc = _status("plvi_loop_window", *structs, qs, out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_loop_window")
        r = {k: a[:1] for k, a in res.items()}
        r.update(rc=rc, past={k: a[1].tolist() for k, a in res.items()})
        return r

    def merge_batch(self, win, n_win, abort_at, matches12, n1, n_queries=None, cap1=None, fill=-7, stream=None,
                    run=True):
        """plvi_loop_bow_merge_batch.  win [q][31], n_win [q], abort_at [q], matches12 [q][6][cap1] and n1 [q] are
        numpy arrays (uploaded) or device addresses (then n_queries and cap1 are given).  Returns matched_mp /
        matched_kf [q][cap1] and num [q], sentinel-filled, plus "past", "dev" and "rc"."""
        self._check_tables()
        dev = self.upload()
        structs = self._structs(lambda g, k: dev[(g, k)].ptr)
        B = len(n1) if n_queries is None else n_queries
        cap1 = np.shape(matches12)[2] if cap1 is None else cap1
        shapes = {"win": (B, LOOP_WIN_MAX), "n_win": (B,), "abort_at": (B,), "matches12": (B, LOOP_BOW_WIN, cap1),
                  "n1": (B,)}
        ins, keep = {}, []
        for k, v in zip(shapes, (win, n_win, abort_at, matches12, n1)):
            if isinstance(v, (int, np.integer)):
                ins[k] = int(v)
                continue
            a = np.ascontiguousarray(v, np.int32)
            if a.shape != shapes[k]:
                raise ValueError(f"{k} has shape {a.shape}, expected {shapes[k]}")
            keep.append(_to_device(a)[0][0])
            ins[k] = keep[-1].ptr
        res = {k: np.full((B + 1, max(cap1, 1)), fill, np.int32) for k in _LOOP_MERGE_OUT}
        res["num"] = np.full(B + 1, fill, np.int32)
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        sb = load().plvi_loop_window_scratch_bytes(B, len(self.pools[0]["bad"]))
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_loop_bow_merge_batch", B, *structs, ins["win"], ins["n_win"], ins["abort_at"],
                           ins["matches12"], ins["n1"], cap1, obuf["matched_mp"].ptr, obuf["matched_kf"].ptr,
                           obuf["num"].ptr, scratch.ptr, sb, s or None)

        def fetch(rc=0):
            _sync()
            full = {k: obuf[k].download(a) for k, a in res.items()}
            r = {k: a[:B] for k, a in full.items()}
            r.update(rc=rc, past={k: a[B].tolist() for k, a in full.items()}, keep=(keep, obuf, scratch),
                     dev={k: b.ptr for k, b in obuf.items()})
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def merge_host(self, win, n_win, abort_at, matches12, n1, fill=-7):
        """One merge through the host form (plvi_loop_bow_merge): win [31], matches12 [6][cap1]."""
        self._check_tables()
        win, m12 = _table(win, np.int32), _table(matches12, np.int32)
        if win.shape != (LOOP_WIN_MAX,):
            raise ValueError(f"win has shape {win.shape}, expected ({LOOP_WIN_MAX},)")
        if m12.ndim != 2 or m12.shape[0] != LOOP_BOW_WIN:
            raise ValueError(f"matches12 has shape {m12.shape}, expected ({LOOP_BOW_WIN}, cap1)")
        cap1 = m12.shape[1]
        tabs = _named_tables(self.kf, self.pools)
        structs = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        one = lambda v: np.array([v], np.int32)  # noqa: E731
        res = {k: np.full((2, max(cap1, 1)), fill, np.int32) for k in _LOOP_MERGE_OUT}
        res["num"] = np.full(2, fill, np.int32)
        rc = _status("plvi_loop_bow_merge", *structs, win, one(n_win), one(abort_at), m12, one(n1), cap1,
                     res["matched_mp"], res["matched_kf"], res["num"])
        if rc < 0:
            raise PlviError(rc, "plvi_loop_bow_merge")
        r = {k: a[:1] for k, a in res.items()}
        r.update(rc=rc, past={k: a[1].tolist() for k, a in res.items()})
        return r


EG_MAX_WIN = COVIS_MAX_CONN + 1  # PLVI_EG_MAX_WIN: longest window
EG_MIN_FEAT = 100                # PLVI_EG_MIN_FEAT: minFeat of OptimizeEssentialGraph
EG_7DOF, EG_4DOF = 0, 1
EG_EDGE_LOOPCONN, EG_EDGE_TREE, EG_EDGE_LOOP, EG_EDGE_COVIS, EG_EDGE_INERTIAL = range(5)
(EG_ERR_WIN, EG_ERR_PTS, EG_ERR_LNS, EG_ERR_QUERY, EG_ERR_VERT, EG_ERR_EDGE, EG_ERR_NO_VERTEX,
 EG_ERR_LC) = (1 << i for i in range(8))

_EG_CULL = ("bad", "init_kf", "mp", "nmp", "ml", "nml", "cand", "n_cand", "kf_id", "prev_kf", "next_kf")
_EG_KF = {"order": np.int32, "map_id": np.int32, "parent": np.int32, "child_off": np.int32, "child": np.int32,
          "loop_off": np.int32, "loop": np.int32, "imu": np.uint8, "cand_w": np.int32, "map_kf": np.int32,
          "map_w": np.int32, "map_n": np.int32}
_EG_FEAT = {"ref_kf": np.int32, "corr_by": np.uint32, "corr_ref": np.int32, "map_id": np.int32}
_EG_CORRECT_LISTS = {"win": "win_cap", "win_sorted": "win_cap", "pts": "pt_cap", "pts_kf": "pt_cap", "lns": "ln_cap",
                     "lns_kf": "ln_cap"}
_EG_CORRECT_N = ("n_win", "n_sorted", "n_pts", "n_lns", "err")
_EG_GRAPH_LISTS = {"vert": "vert_cap", "vert_flags": "vert_cap", "edge_a": "edge_cap", "edge_b": "edge_cap",
                   "edge_kind": "edge_cap"}


class EgKeyframes(ctypes.Structure):
    """plvi_eg_keyframes."""
    _fields_ = [("n_order", _LM_I), ("map_stride", _LM_I)] + [(k, _LM_V) for k in _EG_KF]


class EgFeatures(ctypes.Structure):
    """plvi_eg_features."""
    _fields_ = [(k, _LM_V) for k in _EG_FEAT]


class LoopCorrectOutputs(ctypes.Structure):
    """plvi_loop_correct_outputs."""
    _fields_ = [("win_cap", _LM_I), ("pt_cap", _LM_I), ("ln_cap", _LM_I)] + \
               [(k, _LM_V) for k in ("win", "n_win", "win_sorted", "n_sorted", "pts", "pts_kf", "n_pts", "lns",
                                     "lns_kf", "n_lns", "err")]


class EgOutputs(ctypes.Structure):
    """plvi_eg_outputs."""
    _fields_ = [("vert_cap", _LM_I), ("edge_cap", _LM_I)] + \
               [(k, _LM_V) for k in ("vert", "vert_flags", "n_vert", "edge_a", "edge_b", "edge_kind", "n_edges",
                                     "pt_ref", "ln_ref", "err")]


class EssentialGraph:
    """The integer work of LoopClosing::CorrectLoop[WithLines] and Optimizer::OptimizeEssentialGraph[4DoF] over
    resident tables: the corrected window and the correction owners (plvi_loop_correct), LoopConnections
    (plvi_loop_connections) and the vertices, edges and feature references (plvi_essential_graph).

    ``keyframes``: a dict of numpy arrays named as the fields of plvi_cull_keyframes (bad, mp / nmp, cand / n_cand,
    kf_id, prev_kf, next_kf and optionally init_kf, ml / nml) and of plvi_eg_keyframes (order, cand_w, map_kf /
    map_w / map_n and optionally map_id, parent, child_off / child, loop_off / loop, imu).  ``points`` / ``lines``:
    dicts with bad and optionally ref_kf, corr_by, corr_ref, map_id.  ``rows``: a dict of device addresses cand,
    n_cand, cand_w, map_kf, map_w, map_n and their row length ``stride`` (Covisibility.rows() and .map_rows()),
    which replace those six tables in the device forms: the graph's rows are read in place.

    The ``*_device`` methods run on device copies (``self.dev``; the stamps written by ``correct_device`` are read
    by ``graph_device``), the ``*_host`` methods go through the host forms and update the host arrays in place.
    Each returns a dict of its outputs, sentinel-filled where nothing was written, plus "rc"; the device forms add
    "dev" (the device address of every output) and, with run=False, return (step(stream), fetch()) instead."""

    def __init__(self, keyframes, points, lines=None, rows=None):
        self._lib = load()
        self.kf = {k: _table(keyframes[k], _CULL_KF[k]) for k in _EG_CULL if keyframes.get(k) is not None}
        self.eg = {k: _table(keyframes[k], dt) for k, dt in _EG_KF.items() if keyframes.get(k) is not None}
        feat = lambda p: None if p is None else (  # noqa: E731
            {"bad": _table(p["bad"], np.uint8)},
            {k: _table(p[k], dt) for k, dt in _EG_FEAT.items() if p.get(k) is not None})
        self.pools = [feat(points), feat(lines)]
        self.kf_cap = len(self.kf["bad"])
        self.rows = rows
        self.dev = None

    def _tables(self):
        t = {("kf", k): a for k, a in self.kf.items()}
        t.update({("eg", k): a for k, a in self.eg.items()})
        for g, p in zip(("mp", "ml"), self.pools):
            if p is not None:
                t[(g, "bad")] = p[0]["bad"]
                t.update({("f" + g, k): a for k, a in p[1].items()})
        return t

    def _check_tables(self):
        """Every companion array has the length its table gives it: refused here, before the library reads them."""
        K = self.kf_cap
        _same_len(K, **{"keyframes." + k: a for k, a in self.kf.items()})
        _same_len(K, **{"keyframes." + k: a for k, a in self.eg.items()
                        if k not in ("order", "child_off", "child", "loop_off", "loop")})
        for off, row in (("child_off", "child"), ("loop_off", "loop")):
            if (off in self.eg) != (row in self.eg):
                raise ValueError(f"keyframes.{off} and keyframes.{row} go together")
            if off in self.eg:
                _same_len(K + 1, **{"keyframes." + off: self.eg[off]})
                _same_len(max(int(self.eg[off][K]), 0), **{"keyframes." + row: self.eg[row]})
        if "cand" in self.kf and "cand_w" in self.eg and self.kf["cand"].shape != self.eg["cand_w"].shape:
            raise ValueError("keyframes.cand_w has not the shape of keyframes.cand")
        if "map_kf" in self.eg and self.eg["map_kf"].shape != self.eg.get("map_w", self.eg["map_kf"]).shape:
            raise ValueError("keyframes.map_w has not the shape of keyframes.map_kf")
        for name, p in zip(("points", "lines"), self.pools):
            if p is not None:
                _same_len(len(p[0]["bad"]), **{f"{name}.{k}": a for k, a in p[1].items()})
                if ("corr_by" in p[1]) != ("corr_ref" in p[1]):
                    raise ValueError(f"{name}.corr_by and {name}.corr_ref go together")

    def upload(self):
        if self.dev is None:
            tabs = self._tables()
            self.dev = dict(zip(tabs, _to_device(*tabs.values())[0]))
        return self.dev

    def _n(self, p):
        return 0 if self.pools[p] is None else len(self.pools[p][0]["bad"])

    def _structs(self, ptr, rows=None):
        """(kf, eg, mp, ml, fmp, fml) with the addresses ptr(group, name) gives."""
        width = lambda d, k: d[k].shape[1] if k in d and d[k].ndim == 2 else 0  # noqa: E731
        kf = CullKeyframes(self.kf_cap, width(self.kf, "mp"), width(self.kf, "ml"), width(self.kf, "cand"))
        for k in self.kf:
            setattr(kf, k, ptr("kf", k))
        eg = EgKeyframes(len(self.eg.get("order", ())), width(self.eg, "map_kf"))
        for k in self.eg:
            setattr(eg, k, ptr("eg", k))
        if rows:
            kf.cand_stride = eg.map_stride = rows["stride"]
            kf.cand, kf.n_cand = rows["cand"], rows["n_cand"]
            for k in ("cand_w", "map_kf", "map_w", "map_n"):
                setattr(eg, k, rows[k])
        pools, feats = [], []
        for g, p in zip(("mp", "ml"), self.pools):
            pools.append(None if p is None else LocalMapPool(len(p[0]["bad"]), ptr(g, "bad")))
            feats.append(None if p is None or not p[1] else EgFeatures(**{k: ptr("f" + g, k) for k in p[1]}))
        return (kf, eg, *pools, *feats)

    @staticmethod
    def _outputs(lists, caps, scalars, fill):
        """Pre-filled host outputs: every list one cell longer than its capacity, every count one int (n_edges 5)."""
        res = {k: np.full(caps[c] + 1, fill, np.int32) for k, c in lists.items()}
        res.update({k: np.full(5 if k == "n_edges" else 1, fill, np.int32) for k in scalars})
        return res

    def _stamps(self, fetch_table):
        return {f"{name}_{k}": fetch_table("f" + g, k) for g, name, p in zip(("mp", "ml"), ("pt", "ln"), self.pools)
                if p is not None for k in ("corr_by", "corr_ref") if k in p[1]}

    def _dev_table(self, group, name):
        a = self._tables()[(group, name)]
        return self.dev[(group, name)].download(np.empty_like(a))

    # ---- A
    def _correct_caps(self, win_cap, pt_cap, ln_cap):
        stride = self.rows["stride"] if self.rows else (self.kf["cand"].shape[1] if "cand" in self.kf else 0)
        return dict(win_cap=stride + 1 if win_cap is None else win_cap,
                    pt_cap=max(self._n(0), 1) if pt_cap is None else pt_cap,
                    ln_cap=max(self._n(1), 1) if ln_cap is None else ln_cap)

    def correct_device(self, cur_slot, win_cap=None, pt_cap=None, ln_cap=None, fill=-7, stream=None, run=True):
        """plvi_loop_correct_device.  Returns win, win_sorted, pts, pts_kf, lns, lns_kf (capacity + 1 long), the
        counts and err (one int each), and the stamp tables pt_corr_by, pt_corr_ref, ln_corr_by, ln_corr_ref as
        they stand on the device afterwards."""
        self._check_tables()
        caps = self._correct_caps(win_cap, pt_cap, ln_cap)
        res = self._outputs(_EG_CORRECT_LISTS, caps, _EG_CORRECT_N, fill)
        dev = self.upload()
        structs = self._structs(lambda g, k: dev[(g, k)].ptr, self.rows)
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        out = LoopCorrectOutputs(**caps, **{k: b.ptr for k, b in obuf.items()})
        sb = load().plvi_loop_correct_scratch_bytes(self.kf_cap, self._n(0), self._n(1))
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_loop_correct_device", int(cur_slot), *structs, out, scratch.ptr, sb, s or None)

        def fetch(rc=0):
            _sync()
            r = {k: obuf[k].download(a) for k, a in res.items()}
            r.update(self._stamps(self._dev_table))
            r.update(rc=rc, keep=(obuf, scratch), dev={k: b.ptr for k, b in obuf.items()})
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def correct_host(self, cur_slot, win_cap=None, pt_cap=None, ln_cap=None, fill=-7):
        """plvi_loop_correct: the same dict; the host arrays corr_by / corr_ref are updated in place.  "rc" is
        PLVI_E_CAPACITY when err is not 0; any other refusal raises."""
        self._check_tables()
        caps = self._correct_caps(win_cap, pt_cap, ln_cap)
        res = self._outputs(_EG_CORRECT_LISTS, caps, _EG_CORRECT_N, fill)
        tabs = self._tables()
        structs = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        out = LoopCorrectOutputs(**caps, **{k: a.ctypes.data for k, a in res.items()})
        rc = _status("plvi_loop_correct", int(cur_slot), *structs, out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_loop_correct")
        r = dict(res)
        r.update(self._stamps(lambda g, k: tabs[(g, k)].copy()))
        r["rc"] = rc
        return r

    # ---- B
    @staticmethod
    def _connection_outputs(n_win, lc_cap, fill):
        res = {k: np.full(n_win + 1, fill, np.int32) for k in _COVIS_OUT}
        res["lc_kf"] = np.full((n_win + 1, max(lc_cap, 1)), fill, np.int32)
        res["n_lc"] = np.full(n_win + 1, fill, np.int32)
        res["lc_err"] = np.full(1, fill, np.int32)
        return res

    @staticmethod
    def connections_device(cov, win, lc_cap, fill=-7, stream=None, run=True):
        """plvi_loop_connections_device on the Covisibility `cov` (its resident tables): win is the window as a
        host sequence.  Returns the outputs of the updates by window position (n_counted, n_conn, kf_max, w_max,
        new_parent, err), lc_kf [n_win + 1][lc_cap], n_lc [n_win + 1] and lc_err."""
        win = _table(win, np.int32)
        n_win = len(win)
        res = EssentialGraph._connection_outputs(n_win, lc_cap, fill)
        kf, mp, ml = cov._structs(lambda g, k: cov.dev[(g, k)].ptr)
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        out = CovisOutputs(*[obuf[k].ptr for k in _COVIS_OUT])
        sb = load().plvi_loop_connections_scratch_bytes(n_win, cov.kf_cap, cov.conn_cap)
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_loop_connections_device", cov.h, n_win, win, kf, mp, ml, out, lc_cap,
                           obuf["lc_kf"].ptr, obuf["n_lc"].ptr, obuf["lc_err"].ptr, scratch.ptr, sb, s or None)

        def fetch(rc=0):
            _sync()
            r = {k: obuf[k].download(a) for k, a in res.items()}
            r.update(rc=rc, keep=(obuf, scratch, win), dev={k: b.ptr for k, b in obuf.items()})
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    @staticmethod
    def connections_host(cov, win, lc_cap, fill=-7):
        """plvi_loop_connections: the host arrays first_conn / parent / covis given to cov.set_tables are updated
        in place.  "rc" is PLVI_E_CAPACITY when lc_err is not 0; any other refusal raises."""
        win = _table(win, np.int32)
        n_win = len(win)
        res = EssentialGraph._connection_outputs(n_win, lc_cap, fill)
        tabs = cov._tables()
        kf, mp, ml = cov._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        out = CovisOutputs(*[res[k].ctypes.data for k in _COVIS_OUT])
        rc = _status("plvi_loop_connections", cov.h, n_win, win, kf, mp, ml, out, lc_cap, res["lc_kf"], res["n_lc"],
                     res["lc_err"])
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_loop_connections")
        res["rc"] = rc
        return res

    # ---- C
    def _graph_inputs(self, win, n_win, lc_kf, n_lc, win_cap, lc_cap):
        """win / lc_kf / n_lc as host arrays with their capacities, or device addresses with the capacities given."""
        if isinstance(win, (int, np.integer)):
            return None, (int(win), int(n_win), int(lc_kf), int(n_lc)), win_cap, lc_cap
        win, n_lc = _table(win, np.int32), _table(n_lc, np.int32)
        lc_kf = np.ascontiguousarray(lc_kf, np.int32)
        if lc_kf.ndim != 2 or len(lc_kf) != len(win) or len(n_lc) != len(win):
            raise ValueError(f"lc_kf {lc_kf.shape} / n_lc {n_lc.shape} do not match the window of {len(win)}")
        n = np.array([len(win) if n_win is None else n_win], np.int32)
        return (win, n, lc_kf, n_lc), None, len(win), lc_kf.shape[1]

    def _graph_caps(self, vert_cap, edge_cap):
        return dict(vert_cap=max(self.kf_cap, 1) if vert_cap is None else vert_cap,
                    edge_cap=4 * max(self.kf_cap, 1) if edge_cap is None else edge_cap)

    def _graph_outputs(self, caps, refs, fill):
        res = self._outputs(_EG_GRAPH_LISTS, caps, ("n_vert", "n_edges", "err"), fill)
        if refs:
            res["pt_ref"] = np.full(self._n(0) + 1, fill, np.int32)
            if self.pools[1] is not None:
                res["ln_ref"] = np.full(self._n(1) + 1, fill, np.int32)
        return res

    def graph_device(self, cur_slot, loop_slot, mode, win, n_win, lc_kf, n_lc, win_cap=None, lc_cap=None,
                     vert_cap=None, edge_cap=None, refs=True, fill=-7, stream=None, run=True):
        """plvi_essential_graph_device.  win [win_cap], lc_kf [win_cap][lc_cap] and n_lc [win_cap] are numpy arrays
        (uploaded; n_win None = all of win) or, with n_win, device addresses (then win_cap and lc_cap are given):
        the outputs of correct_device and connections_device in place.  Returns vert, vert_flags, edge_a, edge_b,
        edge_kind (capacity + 1 long), n_vert, n_edges [5], err and, with refs, pt_ref / ln_ref."""
        self._check_tables()
        host, addr, win_cap, lc_cap = self._graph_inputs(win, n_win, lc_kf, n_lc, win_cap, lc_cap)
        caps = self._graph_caps(vert_cap, edge_cap)
        res = self._graph_outputs(caps, refs, fill)
        dev = self.upload()
        structs = self._structs(lambda g, k: dev[(g, k)].ptr, self.rows)
        ibuf = _to_device(*host)[0] if host else ()
        addr = addr or tuple(b.ptr for b in ibuf)
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        out = EgOutputs(**caps, **{k: b.ptr for k, b in obuf.items()})
        sb = load().plvi_essential_graph_scratch_bytes(self.kf_cap, len(self.eg.get("order", ())), win_cap, lc_cap)
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_essential_graph_device", int(cur_slot), int(loop_slot), mode, addr[0], addr[1],
                           win_cap, addr[2], addr[3], lc_cap, *structs, out, scratch.ptr, sb, s or None)

        def fetch(rc=0):
            _sync()
            r = {k: obuf[k].download(a) for k, a in res.items()}
            r.update(rc=rc, keep=(ibuf, obuf, scratch), dev={k: b.ptr for k, b in obuf.items()})
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def graph_host(self, cur_slot, loop_slot, mode, win, n_win, lc_kf, n_lc, vert_cap=None, edge_cap=None, refs=True,
                   fill=-7):
        """plvi_essential_graph with numpy inputs; the same dict.  "rc" is PLVI_E_CAPACITY when err has a bit other
        than EG_ERR_NO_VERTEX; any other refusal raises."""
        self._check_tables()
        host, _, win_cap, lc_cap = self._graph_inputs(win, n_win, lc_kf, n_lc, None, None)
        caps = self._graph_caps(vert_cap, edge_cap)
        res = self._graph_outputs(caps, refs, fill)
        tabs = self._tables()
        structs = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        out = EgOutputs(**caps, **{k: a.ctypes.data for k, a in res.items()})
        rc = _status("plvi_essential_graph", int(cur_slot), int(loop_slot), mode, host[0], host[1], win_cap, host[2],
                     host[3], lc_cap, *structs, out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_essential_graph")
        res["rc"] = rc
        return res


COMPAT_GEMM_FMA = 8       # PLVI_COMPAT_GEMM_FMA (plvi_frustum_params.compat)
COMPAT_SCALEADD_FMA = 16  # PLVI_COMPAT_SCALEADD_FMA (plvi_refresh_params.compat)
REFRESH_POINTS, REFRESH_LINES = 0, 1
REFRESH_NORMAL, REFRESH_DESC = 1, 2
REFRESH_ERR_ROWS, REFRESH_ERR_REF, REFRESH_ERR_LEVEL, REFRESH_ERR_KEYPOINT = 1, 2, 4, 8
REFRESH_MAX_LEVELS = 64  # PLVI_REFRESH_MAX_LEVELS

_REFRESH_FEAT = {"bad": (np.uint8, None), "obs_off": (np.int32, None), "obs_kf": (np.int32, None),
                 "obs_idx": (np.int32, None), "ref_kf": (np.int32, None), **_LM_ROWS}
_REFRESH_COLUMNS = ("normal", "dist", "desc")


class RefreshKeyframes(ctypes.Structure):
    """plvi_refresh_keyframes."""
    _fields_ = [("kf_cap", _LM_I), ("cap", _LM_I)] + [(k, _LM_V) for k in ("bad", "ow", "cnt", "info", "desc")]


class RefreshParams(ctypes.Structure):
    """plvi_refresh_params."""
    _fields_ = [(k, _LM_I) for k in ("kind", "what", "n_levels", "max_obs", "row_cap", "compat")] + \
               [("scale", ctypes.c_float * REFRESH_MAX_LEVELS)]


class RefreshOutputs(ctypes.Structure):
    """plvi_refresh_outputs."""
    _fields_ = [(k, _LM_V) for k in ("normal", "dist", "desc", "state", "best_pos", "best_median", "n_rows", "err")]


class FeatureRefresh:
    """MapPoint / MapLine::UpdateNormalAndDepth and ComputeDistinctiveDescriptors for a list of pool ids over
    resident tables (plvi_feature_refresh[_batch]): the pool columns normal, dist and desc are updated in place.

    ``keyframes``: a dict of numpy arrays of one kind -- bad [K], ow [K][3], cnt [K] (or nmp / nml), info [K][cap]
    (or kp_info / kl_info; points) and desc [K][cap][32] (DESC).  ``features``: a dict with bad, obs_off, obs_kf,
    obs_idx, ref_kf, pos (points) or sep (lines) and the columns normal [n][3], dist [n][2], desc [n][32] --
    the arrays LocalBAWindow and EssentialGraph take plus the pool rows of LocalMap.  ``scale``: mvScaleFactors
    (or mvScaleFactors_l); ``max_obs``: the longest list walked, by default the longest list of the pool.

    ``batch`` runs on device copies (``self.dev``, which keep the refreshed columns), ``host`` goes through the
    host form and updates ``self.feat`` in place.  Both return a dict: state, best_pos, best_median [n_ids],
    n_rows, err, the three columns and "rc"."""

    def __init__(self, keyframes, features, kind=REFRESH_POINTS, scale=(1.0,), max_obs=None, compat=0, cap=None):
        self._lib = load()
        self.kind = int(kind)
        pts = self.kind == REFRESH_POINTS
        pick = lambda *names: next((keyframes[k] for k in names if keyframes.get(k) is not None), None)  # noqa: E731
        self.kf = {"bad": _table(pick("bad"), np.uint8), "ow": _table(pick("ow"), np.float32, 3),
                   "cnt": _table(pick("cnt", "nmp" if pts else "nml"), np.int32),
                   "info": _table(pick("info", "kp_info" if pts else "kl_info"), np.uint8)}
        self.kf = {k: a for k, a in self.kf.items() if a is not None}
        self.kf_cap = len(self.kf["bad"])
        if cap is None:
            cap = self.kf["info"].shape[1] if "info" in self.kf else np.shape(keyframes["desc"])[1]
        self.cap = int(cap)
        if keyframes.get("desc") is not None:
            self.kf["desc"] = np.ascontiguousarray(keyframes["desc"], np.uint8).reshape(-1, self.cap, 32)
        self.feat = {k: _table(features[k], dt, w) for k, (dt, w) in _REFRESH_FEAT.items()
                     if features.get(k) is not None}
        self.scale = np.ascontiguousarray(scale, np.float32)
        if not 1 <= len(self.scale) <= REFRESH_MAX_LEVELS:
            raise ValueError(f"scale has {len(self.scale)} levels, expected 1 to {REFRESH_MAX_LEVELS}")
        self.n = len(self.feat["bad"])
        if max_obs is None:
            max_obs = int(np.diff(self.feat["obs_off"]).max(initial=1)) if self.n else 1
        self.max_obs = max(int(max_obs), 1)
        self.compat = int(compat)
        self.dev = None

    def _check_tables(self):
        """Every companion array has the length its table gives it: refused here, before the library reads them."""
        _same_len(self.kf_cap, **{"keyframes." + k: a for k, a in self.kf.items()})
        for k in ("info", "desc"):
            if k in self.kf and self.kf[k].shape[1:2] != (self.cap,):
                raise ValueError(f"keyframes.{k} has rows of {self.kf[k].shape[1:2]}, expected {self.cap}")
        f, n = self.feat, self.n
        _same_len(n + 1, **{"features.obs_off": f["obs_off"]})
        _same_len(n, **{"features." + k: a for k, a in f.items() if k not in ("obs_off", "obs_kf", "obs_idx")})
        n_obs = int(f["obs_off"][n])
        if len(f["obs_kf"]) < n_obs:
            raise ValueError(f"features.obs_kf has {len(f['obs_kf'])} records, obs_off names {n_obs}")
        _same_len(len(f["obs_kf"]), **{"features.obs_idx": f.get("obs_idx")})

    def _tables(self):
        t = {("kf", k): a for k, a in self.kf.items()}
        t.update({("f", k): a for k, a in self.feat.items()})
        return t

    def upload(self):
        if self.dev is None:
            tabs = self._tables()
            self.dev = dict(zip(tabs, _to_device(*tabs.values())[0]))
        return self.dev

    def _structs(self, ptr):
        kf = RefreshKeyframes(self.kf_cap, self.cap, **{k: ptr("kf", k) for k in self.kf})
        pool = LocalMapPool(self.n, **{k: ptr("f", k) for k in self.feat if k not in ("obs_idx", "ref_kf")})
        feat = BAFeatures(ptr("f", "obs_idx")) if "obs_idx" in self.feat else None
        ref = EgFeatures(ref_kf=ptr("f", "ref_kf")) if "ref_kf" in self.feat else None
        return kf, pool, feat, ref

    def _params(self, what, row_cap, compat):
        p = RefreshParams(self.kind, int(what), len(self.scale), self.max_obs, int(row_cap),
                          self.compat if compat is None else int(compat))
        p.scale[:len(self.scale)] = self.scale.tolist()
        return p

    def rows_of(self, ids):
        """The full length of the observation list plvi_feature_refresh builds for ``ids``: n_rows."""
        ids = np.asarray(ids, np.int64).reshape(-1)
        ok = (ids >= 0) & (ids < self.n)
        idc = np.where(ok, ids, 0)
        ln = np.clip(self.feat["obs_off"][idc + 1].astype(np.int64) - self.feat["obs_off"][idc], 0, self.max_obs)
        return int(np.where(ok & (self.feat["bad"][idc] == 0), ln, 0).sum()) if len(ids) else 0

    @staticmethod
    def _host(n_ids, best, fill):
        res = {"state": np.full(n_ids + 1, fill & 0x7f, np.uint8),  # one cell more than is written
               "n_rows": np.full(1, fill, np.int32), "err": np.full(1, fill, np.int32)}
        if best:
            res.update(best_pos=np.full(n_ids + 1, fill, np.int32), best_median=np.full(n_ids + 1, fill, np.int32))
        return res

    @staticmethod
    def _result(res, n_ids, rc):
        r = {k: (a[:n_ids] if k not in ("n_rows", "err") else int(a[0])) for k, a in res.items()}
        r.update(rc=rc, past={k: a[n_ids].tolist() for k, a in res.items() if k not in ("n_rows", "err")})
        return r

    def batch(self, ids=None, what=REFRESH_NORMAL | REFRESH_DESC, row_cap=None, compat=None, d_ids=None, n_ids=None,
              best=True, fill=-7, stream=None, run=True):
        """plvi_feature_refresh_batch of ``ids`` (a numpy list, or a device address ``d_ids`` of ``n_ids`` ints,
        which needs ``row_cap``).  Adds "dev", the device addresses of the three columns, and "past" (the cell
        after the last id of every per-id output).  run=False returns (step(stream), fetch()) for capture."""
        self._check_tables()
        dev = self.upload()
        structs = self._structs(lambda g, k: dev[(g, k)].ptr)
        keep = []
        if d_ids is None:
            ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
            n_ids = len(ids)
            keep += _to_device(ids)[0]
            d_ids = keep[0].ptr
            if row_cap is None:
                row_cap = self.rows_of(ids)
        params = self._params(what, 0 if row_cap is None else row_cap, compat)
        res = self._host(n_ids, best, fill)
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        cols = {k: dev[("f", k)].ptr if ("f", k) in dev else None for k in _REFRESH_COLUMNS}
        out = RefreshOutputs(**cols, **{k: b.ptr for k, b in obuf.items()})
        sb = load().plvi_feature_refresh_scratch_bytes(n_ids, params.row_cap)
        scratch = DeviceBuffer(sb)

        def step(s=None):
            return _status("plvi_feature_refresh_batch", *structs, params, d_ids, n_ids, out, scratch.ptr, sb, s or None)

        def fetch(rc=0):
            _sync()
            r = self._result({k: obuf[k].download(a) for k, a in res.items()}, n_ids, rc)
            r.update({k: dev[("f", k)].download(np.empty_like(self.feat[k])) for k in _REFRESH_COLUMNS
                      if k in self.feat})
            r.update(dev=cols, keep=(keep, obuf, scratch))
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def host(self, ids, what=REFRESH_NORMAL | REFRESH_DESC, row_cap=None, compat=None, best=True, fill=-7):
        """plvi_feature_refresh with numpy inputs: the columns of ``self.feat`` are updated in place.  "rc" is the
        number of ids with the NORMAL bit, or PLVI_E_CAPACITY when err is not 0; any other refusal raises."""
        self._check_tables()
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        tabs = self._tables()
        structs = self._structs(lambda g, k: tabs[(g, k)].ctypes.data)
        params = self._params(what, self.rows_of(ids) if row_cap is None else row_cap, compat)
        res = self._host(len(ids), best, fill)
        cols = {k: self.feat[k].ctypes.data if k in self.feat else None for k in _REFRESH_COLUMNS}
        out = RefreshOutputs(**cols, **{k: a.ctypes.data for k, a in res.items()})
        rc = _status("plvi_feature_refresh", *structs, params, ids, len(ids), out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_feature_refresh")
        r = self._result(res, len(ids), rc)
        r.update({k: self.feat[k] for k in _REFRESH_COLUMNS if k in self.feat})
        return r


GBA_POINTS, GBA_LINES = 0, 1
GBA_ERR_ORIGIN, GBA_ERR_CYCLE, GBA_ERR_WALK, GBA_ERR_REF = 1, 2, 4, 8

_GBA_KF = {"bad": np.uint8, "order": np.int32, "child_off": np.int32, "child": np.int32, "kf_ba_for": np.uint32}
_GBA_FEAT = {"bad": (np.uint8, None), "ref_kf": (np.int32, None), "map_id": (np.int32, None),
             "ba_for": (np.uint32, None)}
_GBA_POSES = {"kf_ba_for": (np.uint32, None), "has_bef": (np.uint8, None), "tcw_bef": (np.float32, 12),
              "twc": (np.float32, 12)}
_GBA_WALK_LISTS = {"walk": np.int32, "walk_parent": np.int32, "walk_new": np.uint8}
_GBA_WALK_N = ("n_walk", "n_new", "err")


class GbaWalkOutputs(ctypes.Structure):
    """plvi_gba_walk_outputs."""
    _fields_ = [("walk_cap", _LM_I)] + [(k, _LM_V) for k in ("walk", "walk_parent", "walk_new", "n_walk", "n_new",
                                                            "err", "visited")]


class GbaPoses(ctypes.Structure):
    """plvi_gba_poses."""
    _fields_ = [("kf_cap", _LM_I)] + [(k, _LM_V) for k in _GBA_POSES]


class GbaParams(ctypes.Structure):
    """plvi_gba_params."""
    _fields_ = [("kind", _LM_I), ("loop_kf", ctypes.c_uint), ("map", _LM_I), ("compat", _LM_I)]


class GbaCorrectOutputs(ctypes.Structure):
    """plvi_gba_correct_outputs."""
    _fields_ = [(k, _LM_V) for k in ("pos", "sep", "state", "counts", "err")]


class _GbaWalk:
    """plvi_gba_walk[_device] on the tables of a GBAPropagation."""

    def __init__(self, owner):
        self.o = owner

    def _outputs(self, walk_cap, visited, fill):
        o = self.o
        walk_cap = o.kf_cap if walk_cap is None else int(walk_cap)
        if walk_cap < 0:
            raise ValueError(f"walk_cap {walk_cap} is negative")
        res = {k: np.full(walk_cap + 1, fill & 0x7f if dt is np.uint8 else fill, dt)  # one cell past the capacity
               for k, dt in _GBA_WALK_LISTS.items()}
        res.update({k: np.full(1, fill, np.int32) for k in _GBA_WALK_N})
        if visited is True:
            visited = np.zeros(o.kf_cap, np.uint8)
        if visited is not None and visited is not False:
            res["visited"] = _table(visited, np.uint8)
            _same_len(o.kf_cap, visited=res["visited"])
        return walk_cap, res

    def _structs(self, ptr):
        o = self.o
        kf = CullKeyframes(o.kf_cap, 0, 0, 0)
        kf.bad = ptr("kf", "bad")
        eg = EgKeyframes(len(o.kf.get("order", ())), 0)
        for k in ("order", "child_off", "child"):
            if k in o.kf:
                setattr(eg, k, ptr("kf", k))
        return kf, eg

    def batch(self, origins, loop_kf, walk_cap=None, visited=True, scratch=None, fill=-7, stream=None, run=True):
        """plvi_gba_walk_device on the device copies (``owner.dev``; the stamps stay there for ``correct.batch``).
        ``visited``: True = a zeroed table, an array = its start, None = no table.  ``scratch``: (device address,
        bytes) of a block of the caller's.  Returns walk, walk_parent, walk_new (walk_cap + 1 long), n_walk, n_new,
        err, visited, kf_ba_for as it stands on the device, "rc" and "dev"; run=False returns (step(stream),
        fetch()) for capture."""
        o = self.o
        o._check_keyframes()
        origins = _table(origins, np.int32).reshape(-1)
        walk_cap, res = self._outputs(walk_cap, visited, fill)
        sb = load().plvi_gba_walk_scratch_bytes(o.kf_cap)
        if scratch is not None and scratch[1] < sb:
            raise ValueError(f"the scratch block has {scratch[1]} bytes, the walk needs {sb}")
        dev = o.upload()
        structs = self._structs(lambda g, k: dev[(g, k)].ptr)
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        ibuf = _to_device(origins)[0]
        own = None if scratch is not None else DeviceBuffer(sb)
        sptr, sbytes = scratch if scratch is not None else (own.ptr, sb)
        out = GbaWalkOutputs(walk_cap, **{k: b.ptr for k, b in obuf.items()})

        def step(s=None):
            return _status("plvi_gba_walk_device", *structs, ibuf[0].ptr, len(origins), int(loop_kf),
                           dev[("kf", "kf_ba_for")].ptr, out, sptr, sbytes, s or None)

        def fetch(rc=0):
            _sync()
            r = {k: obuf[k].download(a) for k, a in res.items()}
            r["kf_ba_for"] = dev[("kf", "kf_ba_for")].download(np.empty_like(o.kf["kf_ba_for"]))
            r.update(rc=rc, keep=(obuf, ibuf, own), dev={k: b.ptr for k, b in obuf.items()})
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def host(self, origins, loop_kf, walk_cap=None, visited=True, fill=-7):
        """plvi_gba_walk: the same dict; ``owner.kf["kf_ba_for"]`` is stamped in place.  "rc" is n_walk, or
        PLVI_E_CAPACITY when err is not 0; any other refusal raises."""
        o = self.o
        o._check_keyframes()
        origins = _table(origins, np.int32).reshape(-1)
        walk_cap, res = self._outputs(walk_cap, visited, fill)
        structs = self._structs(lambda g, k: o.kf[k].ctypes.data)
        out = GbaWalkOutputs(walk_cap, **{k: a.ctypes.data for k, a in res.items()})
        rc = _status("plvi_gba_walk", *structs, origins, len(origins), int(loop_kf), o.kf["kf_ba_for"], out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_gba_walk")
        r = dict(res)
        r.update(kf_ba_for=o.kf["kf_ba_for"].copy(), rc=rc)
        return r


class _GbaCorrect:
    """plvi_gba_correct[_device] on the pools of a GBAPropagation."""

    def __init__(self, owner):
        self.o = owner

    def _prepare(self, kind, poses):
        o = self.o
        if kind not in (GBA_POINTS, GBA_LINES):
            raise ValueError(f"unknown kind {kind}")
        feat = o.pools[kind]
        if feat is None:
            raise ValueError("no pool of that kind was given")
        o._check_pool(kind)
        poses = {k: _table(poses[k], dt, w) for k, (dt, w) in _GBA_POSES.items() if poses.get(k) is not None}
        if "kf_ba_for" not in poses and "kf_ba_for" in o.kf:
            poses["kf_ba_for"] = o.kf["kf_ba_for"]
        missing = [k for k in _GBA_POSES if k not in poses]
        if missing:
            raise ValueError(f"poses lacks {missing}")
        _same_len(o.kf_cap, **{"poses." + k: a for k, a in poses.items()})
        return feat, poses, "sep" if kind == GBA_LINES else "pos"

    @staticmethod
    def _outputs(n, fill):
        return {"state": np.full(n + 1, fill & 0x7f, np.uint8), "counts": np.full(3, fill, np.int32),
                "err": np.full(1, fill, np.int32)}

    def batch(self, kind, loop_kf, poses, map=0, compat=0, column=None, stamps_on_device=False, fill=-7, stream=None,
              run=True):
        """plvi_gba_correct_device.  ``poses``: a dict has_bef [K], tcw_bef [K][12], twc [K][12] and optionally
        kf_ba_for (default: the keyframe table's; with stamps_on_device the device copy ``walk.batch`` stamped).
        ``column`` None writes the pool's own device column in place, an array is a separate output that starts as
        given.  Returns state (n + 1 long), counts, err, the column under "pos" / "sep", "rc" and "dev" (the
        device addresses of the outputs and of the column)."""
        o = self.o
        feat, poses, col = self._prepare(kind, poses)
        n = len(feat["bad"])
        res = self._outputs(n, fill)
        dev = o.upload()
        g = "ml" if kind == GBA_LINES else "mp"
        pbuf = dict(zip(poses, _to_device(*poses.values())[0]))
        if stamps_on_device:
            pbuf["kf_ba_for"] = dev[("kf", "kf_ba_for")]
        obuf = dict(zip(res, _to_device(*res.values())[0]))
        if column is None:
            cbuf, host_col = dev[(g, col)], np.empty_like(feat[col])
        else:
            host_col = _table(column, *_LM_ROWS[col]).copy()
            _same_len(n, column=host_col)
            cbuf = _to_device(host_col)[0][0]
        pool = LocalMapPool(n, **{k: dev[(g, k)].ptr for k in ("bad", col)})
        ef = EgFeatures(**{k: dev[(g, k)].ptr for k in ("ref_kf", "map_id") if k in feat})
        dposes = GbaPoses(o.kf_cap, **{k: b.ptr for k, b in pbuf.items()})
        params = GbaParams(int(kind), int(loop_kf), int(map), int(compat))
        out = GbaCorrectOutputs(**{col: cbuf.ptr}, **{k: b.ptr for k, b in obuf.items()})

        def step(s=None):
            return _status("plvi_gba_correct_device", pool, ef, dev[(g, "ba_for")].ptr, dev[(g, "pos_gba")].ptr,
                           dposes, params, out, s or None)

        def fetch(rc=0):
            _sync()
            r = {k: obuf[k].download(a) for k, a in res.items()}
            r[col] = cbuf.download(host_col)
            r.update(rc=rc, keep=(pbuf, obuf, cbuf), dev=dict({k: b.ptr for k, b in obuf.items()}, **{col: cbuf.ptr}))
            return r
        if not run:
            return step, fetch
        return fetch(step(stream))

    def host(self, kind, loop_kf, poses, map=0, compat=0, column=None, fill=-7):
        """plvi_gba_correct: the same dict; with ``column`` None the pool's host column is updated in place.  "rc"
        is the number of rows written, or PLVI_E_CAPACITY when err is not 0; any other refusal raises."""
        o = self.o
        feat, poses, col = self._prepare(kind, poses)
        n = len(feat["bad"])
        res = self._outputs(n, fill)
        if column is None:
            host_col = feat[col]
        else:
            host_col = _table(column, *_LM_ROWS[col]).copy()
            _same_len(n, column=host_col)
        pool = LocalMapPool(n, **{k: feat[k].ctypes.data for k in ("bad", col)})
        ef = EgFeatures(**{k: feat[k].ctypes.data for k in ("ref_kf", "map_id") if k in feat})
        dposes = GbaPoses(o.kf_cap, **{k: a.ctypes.data for k, a in poses.items()})
        params = GbaParams(int(kind), int(loop_kf), int(map), int(compat))
        out = GbaCorrectOutputs(**{col: host_col.ctypes.data}, **{k: a.ctypes.data for k, a in res.items()})
        rc = _status("plvi_gba_correct", pool, ef, feat["ba_for"], feat["pos_gba"], dposes, params, out)
        if rc < 0 and rc != PLVI_E_CAPACITY:
            raise PlviError(rc, "plvi_gba_correct")
        r = dict(res)
        r[col] = host_col
        r["rc"] = rc
        return r


class GBAPropagation:
    """The second half of LoopClosing::RunGlobalBundleAdjustment[WithLines] over resident tables: ``walk`` is the
    breadth-first walk of the spanning tree from the map's origins (plvi_gba_walk[_device]), ``correct`` the pass
    over every MapPoint / MapLine (plvi_gba_correct[_device]).  Each has ``.batch`` (device copies, ``self.dev``)
    and ``.host`` (the host forms, updating the host arrays in place).

    ``keyframes``: a dict of numpy arrays bad [K], kf_ba_for [K] (mnBAGlobalForKF) and optionally order,
    child_off [K + 1] / child.  ``points`` / ``lines``: dicts with bad, ref_kf, ba_for (the feature's
    mnBAGlobalForKF), pos_gba ([n][3] float32 / [n][6] float64), the column pos [n][3] / sep [n][6] and optionally
    map_id."""

    def __init__(self, keyframes, points=None, lines=None):
        self._lib = load()
        self.kf = {k: _table(keyframes[k], dt) for k, dt in _GBA_KF.items() if keyframes.get(k) is not None}
        self.kf_cap = len(self.kf["bad"])

        def pool(p, col):
            if p is None:
                return None
            f = {k: _table(p[k], dt, w) for k, (dt, w) in _GBA_FEAT.items() if p.get(k) is not None}
            f[col] = _table(p[col], *_LM_ROWS[col])
            f["pos_gba"] = _table(p["pos_gba"], *_LM_ROWS[col])
            return f
        self.pools = [pool(points, "pos"), pool(lines, "sep")]
        self.dev = None
        self.walk = _GbaWalk(self)
        self.correct = _GbaCorrect(self)

    def _check_keyframes(self):
        """Every companion array has the length its table gives it: refused here, before the library reads them."""
        K = self.kf_cap
        if K < 1:
            raise ValueError("the keyframe table is empty")
        if "kf_ba_for" not in self.kf:
            raise ValueError("keyframes.kf_ba_for is required")
        _same_len(K, **{"keyframes.kf_ba_for": self.kf["kf_ba_for"]})
        if ("child_off" in self.kf) != ("child" in self.kf):
            raise ValueError("keyframes.child_off and keyframes.child go together")
        if "child_off" in self.kf:
            _same_len(K + 1, **{"keyframes.child_off": self.kf["child_off"]})
            _same_len(max(int(self.kf["child_off"][K]), 0), **{"keyframes.child": self.kf["child"]})

    def _check_pool(self, kind):
        f = self.pools[kind]
        missing = [k for k in ("bad", "ref_kf", "ba_for") if k not in f]
        if missing:
            raise ValueError(f"the pool lacks {missing}")
        _same_len(len(f["bad"]), **{("lines." if kind else "points.") + k: a for k, a in f.items()})

    def _tables(self):
        t = {("kf", k): a for k, a in self.kf.items()}
        for g, p in zip(("mp", "ml"), self.pools):
            if p is not None:
                t.update({(g, k): a for k, a in p.items()})
        return t

    def upload(self):
        if self.dev is None:
            tabs = self._tables()
            self.dev = dict(zip(tabs, _to_device(*tabs.values())[0]))
        return self.dev
