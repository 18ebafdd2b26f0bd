"""Fuse on the device: ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:1399-1610, mode 0),
ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1612-1734, mode 1) and LineMatcher::Fuse
(src/LineMatcher.cpp:373-485) as pure searches (csrc/fuse.hip).

Expected values come from tests/native/fuse_ref.cpp, a sequential host restatement in the reference's own order
that also reports an outcome code per candidate.  The CPU part checks the restatement against independent
pure-Python float32 / float64 restatements on seeded general cases (each with at least 20 accepted rows and at
least 5 rows of every rejection code) and asserts the code of every crafted case; the gpu part demands exact
equality of fuse_idx, fuse_dist and nfused.

One crafted line case is weaker than its point counterpart, as found on the CPU: inputs on which
fma(dx, dx, dy*dy) and dx*dx + dy*dy differ in double are easy to find (near the image corner, where pt.x is
small against the midpoint), but the two doubles are one ulp apart and the result is rounded to float before the
compare, so the gate flips only where that ulp straddles a float rounding boundary (about 2^-29 per trial): the
case pins the differing doubles, not a flipped outcome."""
import ctypes
import math
import pathlib
import subprocess

import numpy as np
import pytest

import batch_pack as bp
import plvi
import util

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "fuse_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"

FLAG, DEPTH, IMAGE, DISTANCE, ANGLE, LEVEL, EMPTY_WINDOW, NO_CANDIDATE, THRESHOLD, ACCEPTED, BOUNDS_1, BOUNDS_2 = \
    range(1, 13)
POINT_CODES = set(range(1, 11))
LINE_CODES = set(range(1, 13)) - {IMAGE}
CHUNK = plvi.FUSE_CHUNK

# plvi_fuse_params: 10 floats, th, bf, mode, nlevels, 2 x 16 floats; plvi_fuse_line_params: 8 floats, th, nlevels, 16
assert ctypes.sizeof(plvi.FuseParams) == 4 * (10 + 4 + 32) and ctypes.sizeof(plvi.FuseLineParams) == 4 * (8 + 2 + 16)

f32 = np.float32
_libs = {}
_cache = {}


def ref_lib(nofma=False):
    """The restatement; nofma: the same source with every pinned fused site unfused (-DORACLE_NO_REF_FMA)."""
    if nofma not in _libs:
        so = BUILD / ("libfuse_ref_nofma.so" if nofma else "libfuse_ref.so")
        deps = [SRC, ROOT / "include" / "plvi_frontend.h", ROOT / "oracle" / "ref_fma.h"]
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            so.parent.mkdir(parents=True, exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC"] +
                           (["-DORACLE_NO_REF_FMA"] if nofma else []) + ["-o", str(so), str(SRC)], check=True)
        lib = ctypes.CDLL(str(so))
        V, I = ctypes.c_void_p, ctypes.c_int
        lib.fuse_ref_points.argtypes = [V, V, V, I, V, V, V, V, V, V, V, I, V, V, V]
        lib.fuse_ref_points.restype = I
        lib.fuse_ref_lines.argtypes = [V, V, V, I, V, V, V, V, V, V, V, I, V, V, V]
        lib.fuse_ref_lines.restype = I
        _libs[nofma] = lib
    return _libs[nofma]


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def flipped(desc, nbits, start=0):
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[start:start + nbits] ^= 1
    return np.packbits(bits)


def hamming(a, b):
    return int(np.unpackbits(np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)).sum())


def line_hamming(a, b):
    """LineMatcher::DescriptorDistance: every 32-bit word's count halved and floored."""
    x = np.unpackbits(np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)).reshape(8, 32).sum(1)
    return int((x >> 1).sum())


def inv_level_sigma2(sf):
    """ORBextractor mvInvLevelSigma2 = 1.0f / (mvScaleFactor[i] * mvScaleFactor[i])."""
    out = np.zeros(16, f32)
    for i, s in enumerate(sf):
        if s:
            out[i] = f32(1.0) / f32(f32(s) * f32(s))
    return out


# ====================================================================== points
PT_KEYS = ("flags", "x3dc", "dist", "dot", "level", "mp_desc")
MODE_TH = [(0, 3.0), (1, 4.0), (0, 2.5)]  # Fuse's default th, SearchAndFuse's 4, and a th that is no integer


def fuse_params(c, mode, th):
    p = plvi.FuseParams()
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in c["camera"][:4])
    (p.min_x, p.max_x, p.min_y, p.max_y, p.inv_w, p.inv_h) = c["grid"]
    p.th, p.bf, p.mode = float(th), float(c["bf"]), int(mode)
    p.nlevels = c.get("nlevels", 8)
    for i in range(16):
        p.scale_factors[i] = c["scale_factors"][i]
        p.inv_level_sigma2[i] = c["inv_sigma2"][i]
    return p


def ref_points(c, mode, th, nofma=False):
    """(nfused, fuse_idx, fuse_dist, codes) of the restatement."""
    n_kp, n_pt = len(c["kps"]), len(c["flags"])
    p = fuse_params(c, mode, th)
    arr = {k: np.ascontiguousarray(c[k]) for k in ("kps", "desc") + PT_KEYS}
    ur = None if c.get("uright") is None else np.ascontiguousarray(c["uright"], f32)
    assert arr["dot"].dtype == np.float64 and arr["x3dc"].dtype == f32 and arr["level"].dtype == np.int32
    assert arr["dist"].dtype == f32 and arr["flags"].dtype == np.uint8 and arr["mp_desc"].dtype == np.uint8
    oi, od, code = (np.full(max(n_pt, 1), -7, np.int32) for _ in range(3))
    n = ref_lib(nofma).fuse_ref_points(ctypes.byref(p), _p(arr["kps"]), _p(arr["desc"]), n_kp, _p(ur),
                                       _p(arr["flags"]), _p(arr["x3dc"]), _p(arr["dist"]), _p(arr["dot"]),
                                       _p(arr["level"]), _p(arr["mp_desc"]), n_pt, _p(oi), _p(od), _p(code))
    return n, oi[:n_pt], od[:n_pt], code[:n_pt]


def gpu_points(c, mode, th):
    m = plvi.ORBmatcher()
    args = (fuse_params(c, mode, th), c["kps"], c["desc"], c["flags"], c["x3dc"], c["dist"], c["dot"], c["level"],
            c["mp_desc"])
    return m.FuseSim3(*args) if mode else m.Fuse(*args, uright=c.get("uright"))


def check_gpu_points(c, mode, th):
    ne, ie, de, _ = ref_points(c, mode, th)
    ng, ig, dg = gpu_points(c, mode, th)
    assert ng == ne and np.array_equal(ig, ie) and np.array_equal(dg, de)
    return ne


def points_general(seed, n_kp=400, n_pt=420):
    """util.reloc_case read as (keyframe, candidate points), plus what Fuse adds: the viewing-angle dot product on
    both sides of 0.5 * dist, more points behind the camera, a few predicted levels outside the pyramid, worn
    descriptors, mvuRight
    on about half of the keypoints (for aimed points near the point's own ur) and mvInvLevelSigma2."""
    c = util.reloc_case(seed, n_cur=n_kp, n_kf=n_pt, pre_blocked=0.0)
    rng = np.random.default_rng(seed + 5000)
    c = {"kps": c["cur_kps"], "desc": c["cur_desc"], "grid": c["grid"], "scale_factors": c["scale_factors"],
         "camera": c["camera"], "x3dc": c["x3dc"], "dist": c["dist"], "level": c["level"], "flags": c["kf_flags"],
         "mp_desc": c["mp_desc"]}
    c["x3dc"][rng.random(n_pt) < 0.04, 2] *= -1
    c["dot"] = c["dist"][:, 0].astype(np.float64) * rng.uniform(0.40, 1.0, n_pt)
    out = rng.random(n_pt) < 0.05
    c["level"][out] = rng.choice([-1, 8, 9], int(out.sum()))
    worn = rng.random(n_pt) < 0.15  # descriptors too far from their keypoint's: bestDist above TH_LOW
    bits = np.unpackbits(c["mp_desc"][worn], axis=1)
    bits ^= (rng.random(bits.shape) < 0.2).astype(np.uint8)
    c["mp_desc"][worn] = np.packbits(bits, axis=1)
    c["bf"] = f32(40.0)
    c["inv_sigma2"] = inv_level_sigma2(c["scale_factors"])
    # mvuRight: the right-image column of a point at a depth of its own, or none
    fx, cx = c["camera"][0], c["camera"][2]
    ur = c["kps"]["x"] - c["bf"] / rng.uniform(1.0, 20.0, n_kp).astype(f32)
    with np.errstate(all="ignore"):
        u = fx * c["x3dc"][:, 0] / c["x3dc"][:, 2] + cx
        own = u - c["bf"] / c["x3dc"][:, 2] + rng.normal(0, 1.0, n_pt).astype(f32)
    k = c["kps"]
    for i in range(n_pt):  # points that were aimed at a keypoint: that keypoint sees about the point's ur
        j = int(np.argmin(np.abs(k["x"] - u[i]))) if np.isfinite(u[i]) else 0
        if np.isfinite(own[i]) and abs(k["x"][j] - u[i]) < 6 and rng.random() < 0.6:
            ur[j] = own[i]
    ur[rng.random(n_kp) < 0.45] = -1.0
    c["uright"] = ur.astype(f32)
    return c


POINTS_GENERAL = [21, 23, 29]


def points_general_cached(seed):
    key = ("pts", seed)
    if key not in _cache:
        c = points_general(seed)
        _cache[key] = (c, {mt: ref_points(c, *mt) for mt in MODE_TH})
    return _cache[key]


def py_points(c, mode, th):
    """Pure-Python restatement of ORBmatcher.cc:1399-1610 / :1612-1734 downstream of the caller's inputs."""
    k = c["kps"]
    n_kp, n_pt = len(k), len(c["flags"])
    min_x, max_x, min_y, max_y, inv_w, inv_h = (f32(v) for v in c["grid"])
    cells = [[[] for _ in range(48)] for _ in range(64)]
    for i in range(n_kp):  # AssignFeaturesToGrid / PosInGrid (std::round: half away from zero)
        gx, gy = f32(f32(k["x"][i] - min_x) * inv_w), f32(f32(k["y"][i] - min_y) * inv_h)
        px = int(math.floor(gx + 0.5)) if gx >= 0 else -int(math.floor(-gx + 0.5))
        py = int(math.floor(gy + 0.5)) if gy >= 0 else -int(math.floor(-gy + 0.5))
        if 0 <= px < 64 and 0 <= py < 48:
            cells[px][py].append(i)
    fx, fy, cx, cy = (f32(v) for v in c["camera"][:4])
    sf, isg, bf, thf = c["scale_factors"], c["inv_sigma2"], f32(c["bf"]), f32(th)
    nlev = c.get("nlevels", 8)
    ur_tab = c.get("uright")
    oi, od = np.full(n_pt, -1, np.int32), np.full(n_pt, -1, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n_pt):
            if not c["flags"][i] & 1:
                continue
            X, Y, Z = (f32(t) for t in c["x3dc"][i])
            if Z < 0:
                continue
            invz = f32(f32(1) / Z)
            u, v = f32(f32(f32(fx * X) / Z) + cx), f32(f32(f32(fy * Y) / Z) + cy)
            if not (u >= min_x and u < max_x and v >= min_y and v < max_y):
                continue
            ur = util.fmaf(-bf, invz, u) if np.isfinite(invz) else f32(u - f32(bf * invz))
            d3, dmin, dmax = (f32(t) for t in c["dist"][i])
            if d3 < dmin or d3 > dmax:
                continue
            if float(c["dot"][i]) < 0.5 * float(d3):
                continue
            L = int(c["level"][i])
            if L < 0 or L >= nlev:
                continue
            r = f32(thf * f32(sf[L]))
            x0 = max(0, math.floor(f32(f32(f32(u - min_x) - r) * inv_w)))
            x1 = min(63, math.ceil(f32(f32(f32(u - min_x) + r) * inv_w)))
            y0 = max(0, math.floor(f32(f32(f32(v - min_y) - r) * inv_h)))
            y1 = min(47, math.ceil(f32(f32(f32(v - min_y) + r) * inv_h)))
            if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
                continue
            best, bi = (2 ** 31 - 1 if mode else 256), -1
            for ix in range(x0, x1 + 1):
                for iy in range(y0, y1 + 1):
                    for i2 in cells[ix][iy]:
                        kx, ky = f32(k["x"][i2]), f32(k["y"][i2])
                        if not (abs(f32(kx - u)) < r and abs(f32(ky - v)) < r):
                            continue
                        o = int(k["octave"][i2])
                        if o < L - 1 or o > L:
                            continue
                        if mode == 0:
                            if o < 0:
                                continue
                            ex, ey = f32(u - kx), f32(v - ky)
                            e2 = util.fmaf(ex, ex, f32(ey * ey))
                            kpr = f32(-1) if ur_tab is None else f32(ur_tab[i2])
                            if kpr >= 0:
                                er = f32(ur - kpr)
                                e2 = util.fmaf(er, er, e2)
                                if float(f32(e2 * f32(isg[o]))) > 7.8:
                                    continue
                            elif float(f32(e2 * f32(isg[o]))) > 5.99:
                                continue
                        d = hamming(c["mp_desc"][i], c["desc"][i2])
                        if d < best:
                            best, bi = d, i2
            if best <= 50:
                oi[i], od[i] = bi, best
    return int((oi >= 0).sum()), oi, od


def assert_code_coverage(codes, wanted, what):
    counts = {k: int((codes == k).sum()) for k in wanted}
    assert counts[ACCEPTED] >= 20, (what, counts)
    assert all(n >= 5 for n in counts.values()), (what, counts)
    assert set(np.unique(codes)) <= wanted


@pytest.mark.parametrize("seed", POINTS_GENERAL)
@pytest.mark.parametrize("mt", MODE_TH, ids=["mode0-th3", "mode1-th4", "mode0-th2.5"])
def test_points_restatement_matches_python(seed, mt):
    c, refs = points_general_cached(seed)
    ne, ie, de, codes = refs[mt]
    assert_code_coverage(codes, POINT_CODES, (seed, mt))
    npy, ipy, dpy = py_points(c, *mt)
    assert npy == ne and np.array_equal(ipy, ie) and np.array_equal(dpy, de)
    assert ne == int((codes == ACCEPTED).sum()) and np.array_equal(ie >= 0, codes == ACCEPTED)


def test_points_general_gate_and_modes_matter():
    """The general cases reach what separates the two overloads: the reprojection gate removes candidates in
    mode 0 (rows whose best keypoint differs between the modes at one th), on stereo and on monocular keypoints."""
    c, _ = points_general_cached(POINTS_GENERAL[0])
    a, b = ref_points(c, 0, 3.0), ref_points(c, 1, 3.0)
    differ = np.flatnonzero(a[1] != b[1])
    assert len(differ) >= 5
    mono = dict(c, uright=None)
    assert not np.array_equal(ref_points(mono, 0, 3.0)[1], a[1])


# ---------------------------------------------------------------------- crafted points: unit camera, z = 1
UNIT_CAM = (f32(1), f32(1), f32(0), f32(0), f32(0))
PT_DESC = np.arange(32, dtype=np.uint8) * 11
SF = util.orb_scale_factors()


def kpt(x, y, octave=0):
    k = np.zeros(1, plvi.KEYPOINT_DTYPE)[0]
    k["x"], k["y"], k["octave"], k["size"], k["class_id"] = x, y, octave, 31.0, -1
    return k


def pt(u, v, desc=PT_DESC, level=0, flag=1, z=1.0, dist=(5.0, 2.5, 10.0), dot=5.0):
    return dict(u=u, v=v, desc=desc, level=level, flag=flag, z=z, dist=dist, dot=dot)


def points_case(kps, descs, pts, uright=None, bf=0.0):
    n, m = len(kps), len(pts)
    z = np.array([q["z"] for q in pts], f32).reshape(m)
    with np.errstate(all="ignore"):
        x3 = np.stack([np.array([q["u"] for q in pts], f32).reshape(m) * z,
                       np.array([q["v"] for q in pts], f32).reshape(m) * z, z], 1).astype(f32).reshape(m, 3)
    return {"kps": np.array(kps, plvi.KEYPOINT_DTYPE).reshape(n), "desc": np.array(descs, np.uint8).reshape(n, 32),
            "uright": None if uright is None else np.asarray(uright, f32), "bf": f32(bf),
            "grid": plvi.grid_geometry(752, 480), "scale_factors": SF, "inv_sigma2": inv_level_sigma2(SF),
            "camera": UNIT_CAM, "x3dc": x3, "dist": np.array([q["dist"] for q in pts], f32).reshape(m, 3),
            "dot": np.array([q["dot"] for q in pts], np.float64).reshape(m),
            "level": np.array([q["level"] for q in pts], np.int32).reshape(m),
            "flags": np.array([q["flag"] for q in pts], np.uint8).reshape(m),
            "mp_desc": np.array([q["desc"] for q in pts], np.uint8).reshape(m, 32)}


def one_point(octave=0, **kw):
    """One point at (100, 100) with its own descriptor on a keypoint one pixel away (e2 = 1)."""
    return points_case([kpt(101, 100, octave)], [PT_DESC], [pt(100.0, 100.0, **kw)])


def point_rejection_cases():
    """(name, case, expected code of point 0, modes) at th 3."""
    both = (0, 1)
    edge = lambda u, v: points_case([kpt(u, v)], [PT_DESC], [pt(u, v)])  # noqa: E731
    far = points_case([kpt(300, 300)], [PT_DESC], [pt(100.0, 100.0)])
    inverse = points_case([kpt(101, 100)], [PT_DESC ^ np.uint8(255)], [pt(100.0, 100.0)])
    assert hamming(inverse["desc"][0], PT_DESC) == 256
    cases = [("accepted", one_point(), ACCEPTED, both), ("flag", one_point(flag=0), FLAG, both),
             ("depth", one_point(z=-1.0), DEPTH, both), ("z = 0", one_point(z=0.0), IMAGE, both),
             ("z = -0.0f", one_point(z=-0.0), IMAGE, both),
             ("left of the image", edge(-1.0, 100.0), IMAGE, both), ("u == mnMinX", edge(0.0, 100.0), ACCEPTED, both),
             ("u == mnMaxX", edge(752.0, 100.0), IMAGE, both), ("v == mnMinY", edge(100.0, 0.0), ACCEPTED, both),
             ("v == mnMaxY", edge(100.0, 480.0), IMAGE, both),
             ("too near", one_point(dist=(2.0, 2.5, 10.0)), DISTANCE, both),
             ("too far", one_point(dist=(11.0, 2.5, 10.0)), DISTANCE, both),
             ("dist == min", one_point(dist=(2.5, 2.5, 10.0), dot=2.0), ACCEPTED, both),
             ("dist == max", one_point(dist=(10.0, 2.5, 10.0)), ACCEPTED, both),
             ("angle", one_point(dot=float(np.nextafter(2.5, 0.0))), ANGLE, both),
             ("dot == 0.5 dist", one_point(dot=2.5), ACCEPTED, both),
             ("level -1", one_point(level=-1), LEVEL, both), ("level 0", one_point(level=0), ACCEPTED, both),
             ("level L-1", one_point(octave=7, level=7), ACCEPTED, both),
             ("level L", one_point(octave=7, level=8), LEVEL, both),
             ("empty window", far, EMPTY_WINDOW, both),
             # bestDist starts at 256 in mode 0 (256 < 256 fails: bestIdx stays -1) and at INT_MAX in mode 1
             ("a lone candidate at distance 256, mode 0", inverse, NO_CANDIDATE, (0,)),
             ("a lone candidate at distance 256, mode 1", inverse, THRESHOLD, (1,))]
    for o, code in ((1, NO_CANDIDATE), (2, ACCEPTED), (3, ACCEPTED), (4, NO_CANDIDATE)):  # octave L-2 .. L+1, L = 3
        cases.append((f"octave {o} at level 3", one_point(octave=o, level=3), code, both))
    # octave -1 passes [L-1, L] at level 0; mode 0 would index mvInvLevelSigma2[-1] and takes no candidate
    cases.append(("octave -1 at level 0, mode 1", one_point(octave=-1), ACCEPTED, (1,)))
    cases.append(("octave -1 at level 0, mode 0", one_point(octave=-1), NO_CANDIDATE, (0,)))
    for nbits, code in ((50, ACCEPTED), (51, THRESHOLD)):
        cases.append((f"bestDist {nbits}", points_case([kpt(101, 100)], [flipped(PT_DESC, nbits)],
                                                       [pt(100.0, 100.0)]), code, both))
    # mvuRight -1 / 0 / positive (bf = 0: ur = u = 100): none, er = 100, er = 0.5
    for ur, code in ((-1.0, ACCEPTED), (0.0, NO_CANDIDATE), (99.5, ACCEPTED)):
        cases.append((f"mvuRight {ur}", dict(one_point(), uright=np.array([ur], f32)), code, (0,)))
    cases.append(("mvuRight 0, mode 1", dict(one_point(), uright=np.array([0.0], f32)), ACCEPTED, (1,)))
    return cases


def tie_case():
    """Two keypoints at one distance: index 0 lies in grid column 9, index 1 in column 8, and
    GetFeaturesInArea walks column 8 first -- the first in grid order wins, not the lower index."""
    return points_case([kpt(100, 100, 3), kpt(93.5, 100, 3)], [flipped(PT_DESC, 7), flipped(PT_DESC, 7, 100)],
                       [pt(97.0, 100.0, level=3)])


def gate_edge_case(stereo):
    """The last keypoint position whose chi-square product passes and the first that does not, as two
    one-keypoint cases (mode 0, level 0: mvInvLevelSigma2 = 1).  Mono: ey = 0, kp.x steps away from u;
    stereo: ex = ey = 0, mvuRight steps away from ur = u (bf = 0)."""
    limit = 7.8 if stereo else 5.99
    start = f32(100.0) - f32(math.sqrt(limit)) + f32(1e-3)
    prev = prev_prod = None
    x = start
    for _ in range(4000):
        ex = f32(f32(100.0) - x)
        prod = float(f32(f32(ex * ex) * f32(1.0)))  # the other squares are 0: fma(ex, ex, 0) == ex*ex
        if prod > limit:
            assert prev is not None
            mk = (lambda t: dict(points_case([kpt(100, 100)], [PT_DESC], [pt(100.0, 100.0)]),
                                 uright=np.array([t], f32))) if stereo else \
                (lambda t: points_case([kpt(t, 100)], [PT_DESC], [pt(100.0, 100.0)]))
            return mk(prev), mk(x), prev_prod, prod
        prev, prev_prod, x = x, prod, np.nextafter(x, f32(-np.inf))
    raise AssertionError("no edge found")


def point_contraction_case():
    """An input on which the fused and the unfused e2 round differently and the 5.99 gate flips: points on a
    circle of radius sqrt(5.99) around one keypoint, all in one list (the rows are independent); the first row on
    which the restatement and its unfused build disagree."""
    if "pfma" not in _cache:
        rng = np.random.default_rng(99)
        n = 20000
        phi = rng.uniform(0.2, 1.3, n)
        rad = math.sqrt(5.99) * (1 + rng.uniform(-2e-7, 2e-7, n))
        pts = [pt(float(f32(100 + rad[i] * math.cos(phi[i]))), float(f32(100 + rad[i] * math.sin(phi[i]))))
               for i in range(n)]
        c = points_case([kpt(100, 100)], [PT_DESC], pts)
        a, b = ref_points(c, 0, 3.0)[3], ref_points(c, 0, 3.0, nofma=True)[3]
        rows = np.flatnonzero(a != b)
        assert len(rows), "no row found on which the contraction decides"
        i = int(rows[0])
        _cache["pfma"] = (points_case([kpt(100, 100)], [PT_DESC], [pts[i]]), int(a[i]), int(b[i]))
    return _cache["pfma"]


def test_points_crafted_cases_take_their_branch():
    for name, c, code, modes in point_rejection_cases():
        for mode in modes:
            n, oi, od, codes = ref_points(c, mode, 3.0)
            assert codes[0] == code, (name, mode, codes[0])
            assert (n, oi[0] >= 0) == ((1, True) if code == ACCEPTED else (0, False)), name
    n, oi, od, codes = ref_points(tie_case(), 1, 3.0)
    assert codes[0] == ACCEPTED and oi[0] == 1 and od[0] == 7
    assert ref_points(tie_case(), 0, 3.0)[1][0] == 1
    for stereo in (False, True):
        under, over, p_under, p_over = gate_edge_case(stereo)
        limit = 7.8 if stereo else 5.99
        assert p_under <= limit < p_over and p_over - p_under < 1e-4
        assert ref_points(under, 0, 3.0)[3][0] == ACCEPTED and ref_points(over, 0, 3.0)[3][0] == NO_CANDIDATE
        assert ref_points(over, 1, 3.0)[3][0] == ACCEPTED  # no gate in mode 1
    c, fused, unfused = point_contraction_case()
    assert {fused, unfused} == {ACCEPTED, NO_CANDIDATE}
    assert ref_points(c, 0, 3.0)[3][0] == fused and ref_points(c, 0, 3.0, nofma=True)[3][0] == unfused
    assert py_points(c, 0, 3.0)[0] == (1 if fused == ACCEPTED else 0)


# ====================================================================== lines
ML_KEYS = ("flags", "spc", "epc", "dist", "dot", "level", "ml_desc")
LINE_CAM = (f32(458.654), f32(457.296), f32(367.215), f32(248.375))


def line_params(c, th):
    p = plvi.FuseLineParams()
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in c["camera"][:4])
    p.min_x, p.max_x, p.min_y, p.max_y = (float(v) for v in c["bounds"])
    p.th, p.nlevels = float(th), c.get("nlevels", 8)
    for i in range(16):
        p.scale_factors[i] = c["scale_factors"][i]
    return p


def ref_lines(c, th, nofma=False):
    n_kl, n_ml = len(c["kl"]), len(c["flags"])
    p = line_params(c, th)
    arr = {k: np.ascontiguousarray(c[k]) for k in ("kl", "kl_desc") + ML_KEYS}
    assert arr["dot"].dtype == np.float64 and arr["spc"].dtype == f32 and arr["epc"].dtype == f32
    assert arr["level"].dtype == np.int32 and arr["dist"].dtype == f32 and arr["kl"].dtype == plvi.KEYLINE_DTYPE
    oi, od, code = (np.full(max(n_ml, 1), -7, np.int32) for _ in range(3))
    n = ref_lib(nofma).fuse_ref_lines(ctypes.byref(p), _p(arr["kl"]), _p(arr["kl_desc"]), n_kl, _p(arr["flags"]),
                                      _p(arr["spc"]), _p(arr["epc"]), _p(arr["dist"]), _p(arr["dot"]),
                                      _p(arr["level"]), _p(arr["ml_desc"]), n_ml, _p(oi), _p(od), _p(code))
    return n, oi[:n_ml], od[:n_ml], code[:n_ml]


def gpu_lines(c, th):
    return plvi.LineMatcher.Fuse(line_params(c, th), c["kl"], c["kl_desc"], c["flags"], c["spc"], c["epc"], c["dist"],
                                 c["dot"], c["level"], c["ml_desc"])


def check_gpu_lines(c, th):
    ne, ie, de, _ = ref_lines(c, th)
    ng, ig, dg = gpu_lines(c, th)
    assert ng == ne and np.array_equal(ig, ie) and np.array_equal(dg, de)
    return ne


def lines_general(seed, n_kl=200, n_ml=300, W=752, H=480):
    """Keylines anywhere in the image; MapLines whose projected midpoint lies near a keyline's pt (75 %) with a
    slope around that keyline's `angle` (the reference compares the two directly), descriptors = the keyline's
    with a few bit flips or random, levels = the octave -1 .. +2; the rest anywhere, also across the image
    borders with either endpoint; some behind the camera, out of the distance range or seen from the side."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = LINE_CAM
    kl = np.zeros(n_kl, plvi.KEYLINE_DTYPE)
    kl["pt_x"] = rng.uniform(5, W - 5, n_kl).astype(f32)
    kl["pt_y"] = rng.uniform(5, H - 5, n_kl).astype(f32)
    kl["angle"] = rng.uniform(-1.5, 1.5, n_kl).astype(f32)
    kl["octave"] = np.minimum(rng.geometric(0.4, n_kl) - 1, 7)
    kl["class_id"] = np.arange(n_kl)
    kd = rng.integers(0, 256, (n_kl, 32), dtype=np.uint8)
    near = rng.random(n_ml) < 0.75
    src = rng.integers(0, n_kl, n_ml)
    mx = np.where(near, kl["pt_x"][src] + rng.normal(0, 1.5, n_ml), rng.uniform(-30, W + 30, n_ml))
    my = np.where(near, kl["pt_y"][src] + rng.normal(0, 1.5, n_ml), rng.uniform(-30, H + 30, n_ml))
    s = np.where(near, kl["angle"][src] + rng.uniform(-0.6, 0.06, n_ml), rng.uniform(-2, 2, n_ml))
    hx = np.where(near, rng.uniform(2, 12, n_ml), rng.uniform(2, 60, n_ml)) * rng.choice([-1.0, 1.0], n_ml)
    u1, u2, v1, v2 = mx - hx, mx + hx, my - s * hx, my + s * hx
    # a few lines whose first endpoint is inside and whose second is not
    k = np.flatnonzero(~near)[:12]
    u1[k], u2[k], v1[k], v2[k] = W - 20.0, W + 15.0, rng.uniform(50, 400, len(k)), rng.uniform(50, 400, len(k))
    z1, z2 = rng.uniform(1, 20, n_ml), rng.uniform(1, 20, n_ml)
    z1[rng.random(n_ml) < 0.03] *= -1
    z2[rng.random(n_ml) < 0.03] *= -1
    spc = np.stack([(u1 - cx) * z1 / fx, (v1 - cy) * z1 / fy, z1], 1).astype(f32)
    epc = np.stack([(u2 - cx) * z2 / fx, (v2 - cy) * z2 / fy, z2], 1).astype(f32)
    d3 = (0.5 * (np.abs(z1) + np.abs(z2)) * rng.uniform(1.0, 1.3, n_ml)).astype(f32)
    dist = np.stack([d3, d3 * rng.uniform(0.3, 1.03, n_ml), d3 * rng.uniform(0.97, 3.0, n_ml)], 1).astype(f32)
    lvl = np.where(near, kl["octave"][src] + rng.integers(-1, 3, n_ml), rng.integers(0, 8, n_ml))
    lvl = np.clip(lvl, 0, 7)
    out = rng.random(n_ml) < 0.09
    lvl[out] = rng.choice([-1, 8, 11], int(out.sum()))
    bits = np.unpackbits(kd[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.07).astype(np.uint8)
    md = np.where((near & (rng.random(n_ml) < 0.8))[:, None], np.packbits(bits, axis=1),
                  rng.integers(0, 256, (n_ml, 32), dtype=np.uint8)).astype(np.uint8)
    return {"kl": kl, "kl_desc": kd, "camera": LINE_CAM, "bounds": (f32(0), f32(W), f32(0), f32(H)),
            "scale_factors": SF, "flags": (rng.random(n_ml) < 0.93).astype(np.uint8), "spc": spc, "epc": epc,
            "dist": dist, "dot": d3.astype(np.float64) * rng.uniform(0.42, 1.0, n_ml), "level": lvl.astype(np.int32),
            "ml_desc": md}


LINES_GENERAL = [30, 34, 40]
LINE_TH = [3.0, 2.5]


def lines_general_cached(seed):
    key = ("lines", seed)
    if key not in _cache:
        c = lines_general(seed)
        _cache[key] = (c, {th: ref_lines(c, th) for th in LINE_TH})
    return _cache[key]


def py_lines(c, th, fused=True):
    """Pure-Python restatement of LineMatcher.cpp:373-485 with KeyFrame::GetLinesInArea; fused=False computes
    the midpoint distance without the three double contractions (the object's otherwise)."""
    kl, n_ml = c["kl"], len(c["flags"])
    fx, fy, cx, cy = (f32(v) for v in c["camera"][:4])
    min_x, max_x, min_y, max_y = (f32(v) for v in c["bounds"])
    sf, thf, nlev = c["scale_factors"], f32(th), c.get("nlevels", 8)
    fma = util.fma if fused else (lambda a, b, cc: a * b + cc)
    oi, od = np.full(n_ml, -1, np.int32), np.full(n_ml, -1, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n_ml):
            if not c["flags"][i] & 1:
                continue
            X1, Y1, Z1 = (f32(t) for t in c["spc"][i])
            X2, Y2, Z2 = (f32(t) for t in c["epc"][i])
            if Z1 < 0 or Z2 < 0:
                continue
            iz1, iz2 = f32(f32(1) / Z1), f32(f32(1) / Z2)

            def proj(f, X, iz, c0):
                a = f32(f * X)
                return util.fmaf(a, iz, c0) if np.isfinite(a) and np.isfinite(iz) else f32(f32(a * iz) + c0)
            u1, v1 = proj(fx, X1, iz1, cx), proj(fy, Y1, iz1, cy)
            if u1 < min_x or u1 > max_x or v1 < min_y or v1 > max_y:
                continue
            u2, v2 = proj(fx, X2, iz2, cx), proj(fy, Y2, iz2, cy)
            if u2 < min_x or u2 > max_x or v2 < min_y or v2 > max_y:
                continue
            d3, dmin, dmax = (f32(t) for t in c["dist"][i])
            if d3 < dmin or d3 > dmax:
                continue
            if float(c["dot"][i]) < 0.5 * float(d3):
                continue
            L = int(c["level"][i])
            if L < 0 or L >= nlev:
                continue
            r = f32(thf * f32(sf[L]))
            sx, sy, r2 = float(f32(u1 + u2)), float(f32(v1 + v2)), f32(r * r)
            slope0 = f32(f32(v1 - v2) / f32(u1 - u2))
            best, bi = 2 ** 31 - 1, -1
            for k in range(len(kl)):
                dx, dy = fma(0.5, sx, -float(kl["pt_x"][k])), fma(0.5, sy, -float(kl["pt_y"][k]))
                if f32(fma(dx, dx, dy * dy)) > r2:
                    continue
                if float(f32(slope0 - f32(kl["angle"][k]))) > float(r) * 0.01:
                    continue
                o = int(kl["octave"][k])
                if o < L - 1 or o > L:
                    continue
                d = line_hamming(c["ml_desc"][i], c["kl_desc"][k])
                if d < best:
                    best, bi = d, k
            if best <= 50:
                oi[i], od[i] = bi, best
    return int((oi >= 0).sum()), oi, od


@pytest.mark.parametrize("seed", LINES_GENERAL)
@pytest.mark.parametrize("th", LINE_TH)
def test_lines_restatement_matches_python(seed, th):
    c, refs = lines_general_cached(seed)
    ne, ie, de, codes = refs[th]
    assert_code_coverage(codes, LINE_CODES, (seed, th))
    npy, ipy, dpy = py_lines(c, th)
    assert npy == ne and np.array_equal(ipy, ie) and np.array_equal(dpy, de)
    assert ne == int((codes == ACCEPTED).sum()) and np.array_equal(ie >= 0, codes == ACCEPTED)


# ---------------------------------------------------------------------- crafted lines: unit camera, z = 1
LN_DESC = np.arange(32, dtype=np.uint8) * 13 + 5


def kline(x, y, angle=0.0, octave=0):
    k = np.zeros(1, plvi.KEYLINE_DTYPE)[0]
    k["pt_x"], k["pt_y"], k["angle"], k["octave"] = x, y, angle, octave
    return k


def ml(u1, v1, u2, v2, desc=LN_DESC, level=0, flag=1, z1=1.0, z2=1.0, dist=(5.0, 2.5, 10.0), dot=5.0):
    return dict(u1=u1, v1=v1, u2=u2, v2=v2, desc=desc, level=level, flag=flag, z1=z1, z2=z2, dist=dist, dot=dot)


def lines_case(kls, descs, mls):
    n, m = len(kls), len(mls)
    col = lambda k: np.array([q[k] for q in mls], f32).reshape(m)  # noqa: E731
    with np.errstate(all="ignore"):
        spc = np.stack([col("u1") * col("z1"), col("v1") * col("z1"), col("z1")], 1).astype(f32)
        epc = np.stack([col("u2") * col("z2"), col("v2") * col("z2"), col("z2")], 1).astype(f32)
    return {"kl": np.array(kls, plvi.KEYLINE_DTYPE).reshape(n), "kl_desc": np.array(descs, np.uint8).reshape(n, 32),
            "camera": UNIT_CAM[:4], "bounds": (f32(0), f32(752), f32(0), f32(480)), "scale_factors": SF,
            "spc": spc, "epc": epc, "dist": np.array([q["dist"] for q in mls], f32).reshape(m, 3),
            "dot": np.array([q["dot"] for q in mls], np.float64).reshape(m),
            "level": np.array([q["level"] for q in mls], np.int32).reshape(m),
            "flags": np.array([q["flag"] for q in mls], np.uint8).reshape(m),
            "ml_desc": np.array([q["desc"] for q in mls], np.uint8).reshape(m, 32)}


def one_line(kl=None, desc=LN_DESC, **kw):
    """A level MapLine (90, 100) - (110, 100) (slope -0: (v1 - v2) / (u1 - u2) = 0 / -20) over a keyline at
    its midpoint."""
    return lines_case([kline(100, 100) if kl is None else kl], [desc], [ml(90.0, 100.0, 110.0, 100.0, **kw)])


def line_quirk_desc(dist):
    """A descriptor at LineMatcher distance `dist` from LN_DESC: two flipped bits per unit, in one word each."""
    return flipped(LN_DESC, 2 * dist)


def line_rejection_cases():
    """(name, case, expected code of MapLine 0) at th 3 (r = 3 at level 0, r*r = 9, slope limit 0.03)."""
    at = lambda u1, v1, u2, v2, **kw: lines_case(  # noqa: E731
        [kline(0.5 * (u1 + u2), 0.5 * (v1 + v2), kw.pop("angle", 0.0))], [LN_DESC], [ml(u1, v1, u2, v2, **kw)])
    cases = [("accepted", one_line(), ACCEPTED), ("flag", one_line(flag=0), FLAG),
             ("start point behind the camera", one_line(z1=-1.0), DEPTH),
             ("end point behind the camera", one_line(z2=-1.0), DEPTH),
             ("u1 == mnMinX", at(0.0, 100.0, 20.0, 100.0), ACCEPTED),
             ("u1 below mnMinX", at(-1.0, 100.0, 20.0, 100.0), BOUNDS_1),
             ("u1 == mnMaxX", at(752.0, 100.0, 732.0, 100.0), ACCEPTED),
             ("u1 above mnMaxX", at(753.0, 100.0, 732.0, 100.0), BOUNDS_1),
             ("v1 == mnMinY", at(90.0, 0.0, 110.0, 0.0), ACCEPTED),
             ("v1 == mnMaxY", at(90.0, 480.0, 110.0, 480.0), ACCEPTED),
             ("v1 above mnMaxY", at(90.0, 481.0, 110.0, 470.0, angle=5.0), BOUNDS_1),
             ("u2 == mnMinX", at(20.0, 100.0, 0.0, 100.0), ACCEPTED),
             ("u2 == mnMaxX", at(732.0, 100.0, 752.0, 100.0), ACCEPTED),
             ("u2 above mnMaxX", at(732.0, 100.0, 753.0, 100.0), BOUNDS_2),
             ("v2 == mnMaxY", at(90.0, 470.0, 110.0, 480.0, angle=5.0), ACCEPTED),
             ("v2 below mnMinY", at(90.0, 10.0, 110.0, -1.0), BOUNDS_2),
             ("too near", one_line(dist=(2.0, 2.5, 10.0)), DISTANCE),
             ("too far", one_line(dist=(11.0, 2.5, 10.0)), DISTANCE),
             ("dist == min", one_line(dist=(2.5, 2.5, 10.0), dot=2.0), ACCEPTED),
             ("dist == max", one_line(dist=(10.0, 2.5, 10.0)), ACCEPTED),
             ("angle", one_line(dot=float(np.nextafter(2.5, 0.0))), ANGLE),
             ("dot == 0.5 dist", one_line(dot=2.5), ACCEPTED),
             ("level -1", one_line(level=-1), LEVEL), ("level L", one_line(level=8), LEVEL),
             ("level L-1", one_line(kl=kline(100, 100, 0.0, 7), level=7), ACCEPTED),
             ("octave below", one_line(kl=kline(100, 100, 0.0, 1), level=3), NO_CANDIDATE),
             ("octave L-1", one_line(kl=kline(100, 100, 0.0, 2), level=3), ACCEPTED),
             ("octave above", one_line(kl=kline(100, 100, 0.0, 4), level=3), NO_CANDIDATE),
             ("far keyline", one_line(kl=kline(300, 300)), EMPTY_WINDOW),
             # distance == r*r passes (the compare is >): midpoint 3 px away, r = 3
             ("distance == r*r", one_line(kl=kline(103, 100)), ACCEPTED),
             ("distance above r*r", one_line(kl=kline(float(np.nextafter(f32(103), f32(200))), 100)), EMPTY_WINDOW),
             # slope - angle against r * 0.01 = 0.03, no absolute value
             ("slope above", one_line(kl=kline(100, 100, -0.05)), EMPTY_WINDOW),
             ("slope far below still passes", one_line(kl=kline(100, 100, 1000.0)), ACCEPTED),
             # x1 == x2: +-inf with y1 != y2 (+inf is above every limit, -inf below), NaN with y1 == y2 (passes)
             ("vertical, +inf", lines_case([kline(100, 100)], [LN_DESC], [ml(100.0, 110.0, 100.0, 90.0)]),
              EMPTY_WINDOW),
             ("vertical, -inf", lines_case([kline(100, 100)], [LN_DESC], [ml(100.0, 90.0, 100.0, 110.0)]), ACCEPTED),
             ("a point, NaN", lines_case([kline(100, 100)], [LN_DESC], [ml(100.0, 100.0, 100.0, 100.0)]), ACCEPTED),
             ("quirk distance 50", one_line(desc=line_quirk_desc(50)), ACCEPTED),
             ("quirk distance 51", one_line(desc=line_quirk_desc(51)), THRESHOLD)]
    assert line_hamming(line_quirk_desc(50), LN_DESC) == 50 and hamming(line_quirk_desc(50), LN_DESC) == 100
    return cases


def line_first_minimum_case():
    """Two keylines at one distance: the first in index order wins; odd flips inside a word cost nothing (3
    flipped bits in a word count 1), so a row that ORBmatcher would rank behind ties here."""
    return lines_case([kline(101, 100), kline(100, 100), kline(99, 100)],
                      [flipped(LN_DESC, 4), flipped(LN_DESC, 3), flipped(LN_DESC, 2, 64)],
                      [ml(90.0, 100.0, 110.0, 100.0)])


def line_contraction_case():
    """A MapLine / keyline pair near the image corner on which fma(dx, dx, dy*dy) and dx*dx + dy*dy differ as
    doubles (dx carries more than 26 significant bits where pt.x is small against the midpoint).  Returns
    (case, fused double, unfused double)."""
    if "lfma" not in _cache:
        rng = np.random.default_rng(5)
        for _ in range(2000):
            u1, u2, v1, v2 = (float(f32(t)) for t in (rng.uniform(0.5, 2), rng.uniform(3, 5), rng.uniform(0.5, 2),
                                                     rng.uniform(2.01, 4)))
            px, py = float(f32(rng.uniform(1e-3, 5e-3))), float(f32(rng.uniform(1e-3, 5e-3)))
            dx = util.fma(0.5, float(f32(f32(u1) + f32(u2))), -px)
            dy = util.fma(0.5, float(f32(f32(v1) + f32(v2))), -py)
            a, b = util.fma(dx, dx, dy * dy), dx * dx + dy * dy
            if a != b and f32(a) < 9:
                c = lines_case([kline(px, py, 10.0)], [LN_DESC], [ml(u1, v1, u2, v2)])
                _cache["lfma"] = (c, a, b)
                break
    return _cache["lfma"]


def test_lines_crafted_cases_take_their_branch():
    for name, c, code in line_rejection_cases():
        n, oi, od, codes = ref_lines(c, 3.0)
        assert codes[0] == code, (name, codes[0])
        assert (n, oi[0] >= 0) == ((1, True) if code == ACCEPTED else (0, False)), name
    n, oi, od, codes = ref_lines(line_first_minimum_case(), 3.0)
    assert codes[0] == ACCEPTED and oi[0] == 1 and od[0] == 1
    c, a, b = line_contraction_case()
    assert a != b and abs(a - b) <= 2 * np.spacing(a)
    assert ref_lines(c, 3.0)[3][0] == ACCEPTED and py_lines(c, 3.0)[1][0] == 0
    # (the float conversion absorbs the differing ulp here: the module docstring says why no flip is pinned)
    assert ref_lines(c, 3.0, nofma=True)[3][0] == ACCEPTED and f32(a) == f32(b)


# ====================================================================== GPU
@pytest.mark.gpu
@pytest.mark.parametrize("seed", POINTS_GENERAL)
def test_gpu_points_general_parity(plvi_lib, seed):
    c, refs = points_general_cached(seed)
    for mt in MODE_TH:
        ne, ie, de, _ = refs[mt]
        ng, ig, dg = gpu_points(c, *mt)
        assert ng == ne and np.array_equal(ig, ie) and np.array_equal(dg, de), mt
    mono = dict(c, uright=None)
    assert check_gpu_points(mono, 0, 3.0) >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("n_pt", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7])
def test_gpu_points_chunk_straddle(plvi_lib, n_pt):
    big = points_general(40, 300, 3 * CHUNK + 7)
    c = dict(big, **{k: big[k][:n_pt] for k in PT_KEYS})
    for mode, th in MODE_TH[:2]:
        n = check_gpu_points(c, mode, th)
        assert n >= 5
        # the last row of the list is accepted or not on its own: a live row in the last lane of the last chunk
        last = dict(c, flags=c["flags"].copy())
        last["flags"][:-1] = 0
        check_gpu_points(last, mode, th)


@pytest.mark.gpu
def test_gpu_points_three_times_as_many_points(plvi_lib):
    c = points_general(41, 300, 900)
    for mode, th in MODE_TH:
        assert check_gpu_points(c, mode, th) >= 20
    c = points_general(42, 600, 500)
    for mode, th in MODE_TH[:2]:
        assert check_gpu_points(c, mode, th) >= 20


@pytest.mark.gpu
def test_gpu_points_crafted(plvi_lib):
    for name, c, _, modes in point_rejection_cases():
        for mode in modes:
            check_gpu_points(c, mode, 3.0)
    for mode in (0, 1):
        check_gpu_points(tie_case(), mode, 3.0)
    for stereo in (False, True):
        under, over, _, _ = gate_edge_case(stereo)
        for mode in (0, 1):
            check_gpu_points(under, mode, 3.0)
            check_gpu_points(over, mode, 3.0)
    c, fused, _ = point_contraction_case()
    assert check_gpu_points(c, 0, 3.0) == (1 if fused == ACCEPTED else 0)
    check_gpu_points(c, 1, 3.0)


@pytest.mark.gpu
def test_gpu_points_degenerate(plvi_lib):
    case = points_general(9, 60, 5)
    for n_pt in (0, 1, 5):
        c = dict(case, **{k: case[k][:n_pt] for k in PT_KEYS})
        for mode in (0, 1):
            check_gpu_points(c, mode, 3.0)
    c = dict(case, kps=case["kps"][:0], desc=case["desc"][:0], uright=case["uright"][:0])  # no keypoints
    for mode in (0, 1):
        n, oi, od = gpu_points(c, mode, 3.0)
        assert n == 0 and (oi == -1).all() and (od == -1).all() and len(oi) == 5
        assert ref_points(c, mode, 3.0)[0] == 0
    p = fuse_params(case, 0, 3.0)
    for field, value in (("mode", 2), ("nlevels", 0), ("nlevels", 17)):
        bad = fuse_params(case, 0, 3.0)
        setattr(bad, field, value)
        with pytest.raises(RuntimeError):
            plvi.ORBmatcher()._fuse(value if field == "mode" else 0, bad, case["kps"], case["desc"], case["flags"],
                                    case["x3dc"], case["dist"], case["dot"], case["level"], case["mp_desc"], None)
    # more keypoints than the device grid builder takes
    rc = plvi_lib.plvi_fuse_points(ctypes.byref(p), _p(case["kps"]), _p(case["desc"]), 8193, None, _p(case["flags"]),
                                   _p(case["x3dc"]), _p(case["dist"]), _p(case["dot"]), _p(case["level"]),
                                   _p(case["mp_desc"]), 5, None, None)
    assert rc == plvi.PLVI_E_BADARG


def _points_poison(c):
    """Padding rows of the point tables: aimed exactly at keypoints, with those keypoints' own descriptor and
    octave, in range and in view -- a row read past the count is accepted."""
    idx = np.flatnonzero(bp.ingrid_mask(c, "kps"))
    a = bp._aimed(c, "kps", "desc", idx)
    n = len(a["octave"])
    return {"flags": np.ones(n, np.uint8), "x3dc": a["x3dc"], "level": a["octave"], "mp_desc": a["mp_desc"],
            "dist": np.tile(np.array([5.0, 2.5, 10.0], f32), (n, 1)), "dot": np.full(n, 5.0, np.float64)}


POINTS_KF = {"kps": bp.ingrid("kps"), "desc": bp.own("mp_desc"), "uright": bp.const(-1.0, f32)}
POINTS_PT = bp._spec(_points_poison, PT_KEYS)


@pytest.mark.gpu
def test_gpu_points_batch_of_four(plvi_lib):
    kc, pc = 600, 3 * CHUNK + 7
    sizes = [(kc, pc), (520, CHUNK), (300, CHUNK + 1), (410, 1)]
    cases = [points_general(80 + i, a, b) for i, (a, b) in enumerate(sizes)]
    P = len(cases)
    b = {**bp.pack_keyed(cases, kc, POINTS_KF), **bp.pack_keyed(cases, pc, POINTS_PT)}
    dev = bp.Device()
    dk = dev.up(b["kps"])
    # pair 0 fills both tables: its counts are given above the capacities and must read as clamped
    dn = dev.up(bp.counts_array([len(c["kps"]) for c in cases], {0: kc + 7}))
    dpn = dev.up(bp.counts_array([len(c["flags"]) for c in cases], {0: pc + 1000, 3: -2}))  # pair 3: reads as 0
    off, idx = bp.assign_grid(dev, dk, dn, kc, P, cases[0]["grid"], [c["kps"] for c in cases])
    kf = [dk.value, dev.up(b["desc"]).value, dn.value, dev.up(b["uright"]).value, off.value, idx.value]
    pts = [dev.up(b[k]).value for k in PT_KEYS] + [dpn.value]
    oi, get_i = dev.canary(P + bp.SLACK, pc)
    od, get_d = dev.canary(P + bp.SLACK, pc)
    nf, get_n = dev.canary(P + bp.SLACK)
    no_points = {**cases[3], **{k: cases[3][k][:0] for k in PT_KEYS}}
    for mode, th in MODE_TH[:2]:
        prm = fuse_params(cases[0], mode, th)
        refs = [ref_points(c, mode, th) for c in cases[:3]] + [ref_points(no_points, mode, th)]
        assert refs[0][0] >= 20 and refs[1][0] >= 5 and refs[3][0] == 0
        # twice into the same nfused buffer, never zeroed by the caller (it holds the canary, then the counts)
        for _ in range(2):
            plvi.fuse_points_batch(P, prm, kf, kc, pts, pc, oi.value, od.value, nf.value)
            bp.check_rows(get_i(), [r[1] for r in refs], "fuse_points fuse_idx")
            bp.check_rows(get_d(), [r[2] for r in refs], "fuse_points fuse_dist")
            bp.check_counts(get_n(), [r[0] for r in refs], "fuse_points nfused")
    # refused before any launch: more workgroups than a grid dimension holds; a bad mode; kp_cap above 65535
    before = (get_i(), get_n())
    V = ctypes.c_void_p
    kfa = [V(kf[0]), V(kf[1]), V(kf[2])]
    rest = [V(x) for x in kf[3:]] + [V(x) for x in pts]
    call = plvi_lib.plvi_fuse_points_batch
    assert call(1 << 20, ctypes.byref(prm), *kfa, kc, *rest, 1 << 30, oi, od, nf, None) == plvi.PLVI_E_CAPACITY
    assert call(P, ctypes.byref(prm), *kfa, 65536, *rest, pc, oi, od, nf, None) == plvi.PLVI_E_BADARG
    assert call(P, ctypes.byref(prm), *kfa, kc, *rest, 0, oi, od, nf, None) == plvi.PLVI_E_BADARG
    assert call(-1, ctypes.byref(prm), *kfa, kc, *rest, pc, oi, od, nf, None) == plvi.PLVI_E_BADARG
    assert call(P, ctypes.byref(prm), *kfa, kc, *rest, pc, oi, None, nf, None) == plvi.PLVI_E_BADARG
    prm.mode = 2
    assert call(P, ctypes.byref(prm), *kfa, kc, *rest, pc, oi, od, nf, None) == plvi.PLVI_E_BADARG
    assert call(0, ctypes.byref(fuse_params(cases[0], 0, 3.0)), *([None] * 3), 1, *([None] * 10), 1, None, None, None,
                None) == plvi.PLVI_OK
    assert np.array_equal(get_i(), before[0]) and np.array_equal(get_n(), before[1])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", LINES_GENERAL)
def test_gpu_lines_general_parity(plvi_lib, seed):
    c, refs = lines_general_cached(seed)
    for th in LINE_TH:
        ne, ie, de, _ = refs[th]
        ng, ig, dg = gpu_lines(c, th)
        assert ng == ne and np.array_equal(ig, ie) and np.array_equal(dg, de), th


@pytest.mark.gpu
@pytest.mark.parametrize("n_ml", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7])
def test_gpu_lines_chunk_straddle(plvi_lib, n_ml):
    big = lines_general(50, 100 + n_ml % 7, 3 * CHUNK + 7)
    c = dict(big, **{k: big[k][:n_ml] for k in ML_KEYS})
    assert check_gpu_lines(c, 3.0) >= 5
    last = dict(c, flags=c["flags"].copy())
    last["flags"][:-1] = 0
    check_gpu_lines(last, 3.0)


@pytest.mark.gpu
def test_gpu_lines_crafted(plvi_lib):
    for name, c, _ in line_rejection_cases():
        check_gpu_lines(c, 3.0)
    check_gpu_lines(line_first_minimum_case(), 3.0)
    assert check_gpu_lines(line_contraction_case()[0], 3.0) == 1
    assert check_gpu_lines(lines_general(51, 300, 120), 3.0) >= 20  # more keylines than one staging stride


@pytest.mark.gpu
def test_gpu_lines_degenerate(plvi_lib):
    case = lines_general(9, 40, 5)
    for n_ml in (0, 1, 5):
        check_gpu_lines(dict(case, **{k: case[k][:n_ml] for k in ML_KEYS}), 3.0)
    c = dict(case, kl=case["kl"][:0], kl_desc=case["kl_desc"][:0])
    n, oi, od = gpu_lines(c, 3.0)
    assert n == 0 and (oi == -1).all() and (od == -1).all() and len(oi) == 5 and ref_lines(c, 3.0)[0] == 0
    bad = line_params(case, 3.0)
    bad.nlevels = 17
    with pytest.raises(RuntimeError):
        plvi.LineMatcher.Fuse(bad, case["kl"], case["kl_desc"], case["flags"], case["spc"], case["epc"], case["dist"],
                              case["dot"], case["level"], case["ml_desc"])


def _aimed_lines(c):
    """Padding rows of the MapLine tables: copies of the pair's own accepted MapLines (a row read past the
    count is accepted again)."""
    keep = np.flatnonzero(ref_lines(c, 3.0)[3] == ACCEPTED) if len(c["flags"]) else np.zeros(0, np.int64)
    return {k: np.asarray(c[k])[keep] for k in ML_KEYS}


LINES_KF = {"kl": bp.own("kl"), "kl_desc": bp.own("ml_desc")}
LINES_ML = bp._spec(_aimed_lines, ML_KEYS)


@pytest.mark.gpu
def test_gpu_lines_batch_of_four(plvi_lib):
    kc, mc = 300, 3 * CHUNK + 7
    sizes = [(kc, mc), (100, CHUNK), (220, CHUNK + 1), (150, 1)]
    cases = [lines_general(90 + i, a, b) for i, (a, b) in enumerate(sizes)]
    P = len(cases)
    b = {**bp.pack_keyed(cases, kc, LINES_KF), **bp.pack_keyed(cases, mc, LINES_ML)}
    dev = bp.Device()
    dn = dev.up(bp.counts_array([len(c["kl"]) for c in cases], {0: kc + 7}))
    dmn = dev.up(bp.counts_array([len(c["flags"]) for c in cases], {0: mc + 1000, 3: -2}))
    kf = [dev.up(b["kl"]).value, dev.up(b["kl_desc"]).value, dn.value]
    mls = [dev.up(b[k]).value for k in ML_KEYS] + [dmn.value]
    oi, get_i = dev.canary(P + bp.SLACK, mc)
    od, get_d = dev.canary(P + bp.SLACK, mc)
    nf, get_n = dev.canary(P + bp.SLACK)
    no_lines = {**cases[3], **{k: cases[3][k][:0] for k in ML_KEYS}}
    prm = line_params(cases[0], 3.0)
    refs = [ref_lines(c, 3.0) for c in cases[:3]] + [ref_lines(no_lines, 3.0)]
    assert refs[0][0] >= 20 and refs[1][0] >= 5 and refs[3][0] == 0
    for _ in range(2):  # back to back into the same nfused buffer
        plvi.fuse_lines_batch(P, prm, kf, kc, mls, mc, oi.value, od.value, nf.value)
        bp.check_rows(get_i(), [r[1] for r in refs], "fuse_lines fuse_idx")
        bp.check_rows(get_d(), [r[2] for r in refs], "fuse_lines fuse_dist")
        bp.check_counts(get_n(), [r[0] for r in refs], "fuse_lines nfused")
    # the LDS rule: 48 * kl_cap bytes against 160 KB, refused before any launch
    before = (get_i(), get_n())
    V = ctypes.c_void_p
    kfa = [V(kf[0]), V(kf[1]), V(kf[2])]
    rest = [V(x) for x in mls]
    call = plvi_lib.plvi_fuse_lines_batch
    assert call(P, ctypes.byref(prm), *kfa, 3500, *rest, mc, oi, od, nf, None) == plvi.PLVI_E_CAPACITY
    assert call(1 << 20, ctypes.byref(prm), *kfa, kc, *rest, 1 << 30, oi, od, nf, None) == plvi.PLVI_E_CAPACITY
    assert call(P, ctypes.byref(prm), *kfa, 0, *rest, mc, oi, od, nf, None) == plvi.PLVI_E_BADARG
    assert call(P, ctypes.byref(prm), *kfa, kc, *rest, mc, None, od, nf, None) == plvi.PLVI_E_BADARG
    prm.nlevels = 0
    assert call(P, ctypes.byref(prm), *kfa, kc, *rest, mc, oi, od, nf, None) == plvi.PLVI_E_BADARG
    assert np.array_equal(get_i(), before[0]) and np.array_equal(get_n(), before[1])
