"""The loop-closing matchers: ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)
(src/ORBmatcher.cc:823-963, single-camera branch) and both ORBmatcher::SearchByProjection(pKF, Scw, ...)
overloads (:473-586 and :588-704), the three matcher calls of LoopClosing::DetectCommonRegionsFromBoW /
FindMatchesByProjection.

The expected values come from tests/native/loop_match_ref.cpp, a sequential host restatement built here with
-ffp-contract=off.  It also returns why each KF1 keypoint / each candidate point ended as it did (the BOW_* and
SIM3_* codes below), so every crafted case proves from the restatement alone that its input takes the branch it
is named for; the restatement itself is checked against an independent pure-Python float32 restatement on
general cases (the method of tests/test_reloc.py).  The gpu tests then compare the HIP result with the
restatement exactly (match table and count).

The crafted projection cases use fx = fy = 1, cx = cy = 0 and z = 1, so that u = x and v = y exactly in both
projection forms; the general cases use a real camera.
"""
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
SRC = ROOT / "tests" / "native" / "loop_match_ref.cpp"
SO = ROOT / "tests" / "native" / "_build" / "libloop_match_ref.so"

NOT_LIVE, NO_SHARED_NODE, BOW_NO_CANDIDATE, BOW_TH_LOW, RATIO, BOW_ACCEPTED, HISTOGRAM = range(1, 8)
ALL_BOW_CODES = set(range(1, 8))
FLAG, DEPTH, IMAGE, DISTANCE, ANGLE, LEVEL, EMPTY_WINDOW, NO_CANDIDATE, THRESHOLD, ACCEPTED = range(1, 11)
ALL_SIM3_CODES = set(range(1, 11))

# plvi_sim3_proj_params: 10 floats, th, ratio_hamming, projection, nlevels, 16 floats
assert ctypes.sizeof(plvi.Sim3ProjParams) == 4 * (10 + 4 + 16)

f32 = np.float32
_ref = None


def ref_lib():
    global _ref
    if _ref is None:
        deps = [SRC, ROOT / "include" / "plvi_frontend.h", ROOT / "oracle" / "ref_fma.h"]
        if not SO.exists() or SO.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            SO.parent.mkdir(parents=True, exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                            "-o", str(SO), str(SRC)], check=True)
        lib = ctypes.CDLL(str(SO))
        V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        lib.loop_ref_bow_kf.argtypes = [F, I, V, V, V, I, V, V, I, V, V, V, V, I, V, V, I, V, V, V]
        lib.loop_ref_bow_kf.restype = I
        lib.loop_ref_sim3_projection.argtypes = [V, V, V, I, V, V, V, V, V, V, V, I, V, V, V]
        lib.loop_ref_sim3_projection.restype = I
        _ref = lib
    return _ref


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def flipped(desc, nbits, start=0):
    """A copy of the 32-byte row with bits [start, start + nbits) flipped."""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[start:start + nbits] ^= 1
    return np.packbits(bits)


def hamming(a, b):
    return int(np.unpackbits(np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)).sum())


# ====================================================================== SearchByBoW(KF, KF)
def bow_case(desc1, fv1, desc2, fv2, angle1=None, angle2=None, live1=None, live2=None, nnratio=0.6, ori=False):
    n1, n2 = len(desc1), len(desc2)
    return dict(desc1=np.array(desc1, np.uint8).reshape(n1, 32), desc2=np.array(desc2, np.uint8).reshape(n2, 32),
                angle1=np.zeros(n1, f32) if angle1 is None else np.asarray(angle1, f32),
                angle2=np.zeros(n2, f32) if angle2 is None else np.asarray(angle2, f32),
                live1=np.ones(n1, np.uint8) if live1 is None else np.asarray(live1, np.uint8),
                live2=np.ones(n2, np.uint8) if live2 is None else np.asarray(live2, np.uint8),
                fv1=fv1, fv2=fv2, nnratio=nnratio, ori=ori)


def ref_bow(c):
    """(nmatches, matches12, codes) of the restatement."""
    n1, n2 = len(c["desc1"]), len(c["desc2"])
    a, ao, ai = plvi.feature_vector_csr(c["fv1"])
    b, bo, bi = plvi.feature_vector_csr(c["fv2"])
    m = np.full(max(n1, 1), -7, np.int32)
    codes = np.zeros(max(n1, 1), np.int32)
    n = ref_lib().loop_ref_bow_kf(c["nnratio"], int(c["ori"]), _p(c["desc1"]), _p(c["angle1"]), _p(c["live1"]), n1,
                                  _p(a), _p(ao), len(a), _p(ai), _p(c["desc2"]), _p(c["angle2"]), _p(c["live2"]), n2,
                                  _p(b), _p(bo), len(b), _p(bi), _p(m), _p(codes))
    return n, m[:n1], codes[:n1]


def gpu_bow(c):
    return plvi.ORBmatcher(c["nnratio"], c["ori"]).SearchByBoWKF(c["desc1"], c["angle1"], c["live1"], c["fv1"],
                                                                 c["desc2"], c["angle2"], c["live2"], c["fv2"])


def check_gpu_bow(c):
    ne, me, _ = ref_bow(c)
    ng, mg = gpu_bow(c)
    assert ng == ne and np.array_equal(mg, me)


def _three_maxima(counts):
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for b, c in enumerate(counts):
        if c > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, c, i2, i1, b
        elif c > m2:
            m3, m2, i3, i2 = m2, c, i2, b
        elif c > m3:
            m3, i3 = c, b
    if m2 < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif m3 < f32(0.1) * f32(m1):
        i3 = -1
    return i1, i2, i3


def py_bow(c):
    """Pure-Python restatement of ORBmatcher.cc:823-963: the FeatureVectors as sorted dicts, numpy float32
    where the reference uses float."""
    n1, n2 = len(c["desc1"]), len(c["desc2"])
    m = np.full(n1, -1, np.int32)
    matched2 = [False] * n2
    hist = [[] for _ in range(30)]
    nm = 0
    k1, k2 = sorted(c["fv1"]), sorted(c["fv2"])
    a = b = 0
    while a < len(k1) and b < len(k2):
        if k1[a] == k2[b]:
            for idx1 in c["fv1"][k1[a]]:
                if not c["live1"][idx1]:
                    continue
                b1, bi, b2 = 256, -1, 256
                for idx2 in c["fv2"][k2[b]]:
                    if matched2[idx2] or not c["live2"][idx2]:
                        continue
                    d = hamming(c["desc1"][idx1], c["desc2"][idx2])
                    if d < b1:
                        b2, b1, bi = b1, d, idx2
                    elif d < b2:
                        b2 = d
                if b1 < 50 and f32(b1) < f32(c["nnratio"]) * f32(b2):
                    m[idx1] = bi
                    matched2[bi] = True
                    nm += 1
                    if c["ori"]:
                        rot = f32(c["angle1"][idx1] - c["angle2"][bi])
                        if rot < 0:
                            rot = f32(rot + f32(360))
                        q = int(math.floor(f32(rot * f32(1.0 / 30)) + 0.5))  # roundf, q >= 0
                        hist[0 if q == 30 else q].append(idx1)
            a += 1
            b += 1
        elif k1[a] < k2[b]:
            while a < len(k1) and k1[a] < k2[b]:  # lower_bound
                a += 1
        else:
            while b < len(k2) and k2[b] < k1[a]:
                b += 1
    if c["ori"]:
        keep = _three_maxima([len(h) for h in hist])
        for q in range(30):
            if q not in keep:
                for idx1 in hist[q]:
                    m[idx1] = -1
                    nm -= 1
    return nm, m


def bow_general(seed, n1=300, n2=300, ori=True, nnratio=0.75):
    """About 24 nodes per side (20 shared, private ones in between: both lower_bound jumps), planted pairs at
    distances 0..61 around TH_LOW, keypoints that compete for the same KF2 keypoint inside a node, a global
    rotation with outliers, 10 % of either side without a live MapPoint."""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    a1, a2 = rng.uniform(0, 360, n1).astype(f32), rng.uniform(0, 360, n2).astype(f32)
    nodes1 = list(range(100, 140, 2)) + [201, 203, 205, 207]
    nodes2 = list(range(100, 140, 2)) + [131, 133, 300, 301]
    shared = nodes1[:20]
    node1, node2 = rng.choice(nodes1, n1), rng.choice(nodes2, n2)
    ntrue = 2 * min(n1, n2) // 3
    i1s, i2s = rng.permutation(n1)[:ntrue], rng.permutation(n2)[:ntrue]
    for j, (i1, i2) in enumerate(zip(i1s, i2s)):
        node1[i1] = node2[i2] = rng.choice(shared)
        d1[i1] = flipped(d2[i2], int(rng.integers(0, 62)), int(rng.integers(0, 190)))
        a2[i2] = (a1[i1] - (rng.uniform(-5, 5) if j % 8 else rng.uniform(0, 360))) % 360
    for j in range(0, ntrue - 1, 6):  # the next planted KF1 keypoint aims at the same KF2 keypoint instead
        i1b = i1s[j + 1]
        node1[i1b] = node1[i1s[j]]
        d1[i1b] = flipped(d2[i2s[j]], int(rng.integers(0, 30)), 200)
    live1 = (rng.uniform(size=n1) < 0.9).astype(np.uint8)
    live2 = (rng.uniform(size=n2) < 0.9).astype(np.uint8)
    fv1 = {int(n): [int(i) for i in rng.permutation(np.flatnonzero(node1 == n))] for n in nodes1}
    fv2 = {int(n): [int(i) for i in rng.permutation(np.flatnonzero(node2 == n))] for n in nodes2}
    fv1[150], fv2[150], fv1[99], fv2[400] = [], [], [], []  # empty lists, shared and private
    return bow_case(d1, fv1, d2, fv2, a1, a2, live1, live2, nnratio, ori)


BOW_GENERAL = [dict(seed=41, ori=True), dict(seed=42, ori=False), dict(seed=43, ori=True, nnratio=0.9)]
_cache = {}


def bow_general_cached(i):
    if ("bow", i) not in _cache:
        c = bow_general(**BOW_GENERAL[i])
        _cache["bow", i] = (c, ref_bow(c))
    return _cache["bow", i]


BASE = np.arange(32, dtype=np.uint8) * 7


def bow_threshold_case(nbits):
    """One candidate at distance nbits: bestDist2 stays 256."""
    return bow_case([BASE], {3: [0]}, [flipped(BASE, nbits)], {3: [0]})


def bow_ratio_case(best, second, nnratio=0.9):
    return bow_case([BASE], {3: [0]}, [flipped(BASE, second, 100), flipped(BASE, best)], {3: [0, 1]}, nnratio=nnratio)


def bow_tie_case(order):
    """Three KF2 keypoints at distance 10 (different bits), listed in `order`; nnratio > 1 lets a tie pass."""
    d2 = [flipped(BASE, 10, 0), flipped(BASE, 10, 40), flipped(BASE, 10, 80)]
    return bow_case([BASE], {7: [0]}, d2, {7: list(order)}, nnratio=1.2)


def bow_taken_case(second_choice):
    """KF1 #0 (distance 2) and #1 (distance 1) both have KF2 #0 as their best; #0 comes first in the node's
    list and takes it.  #1 then falls to KF2 #1 at distance 10 (second_choice) or finds the node empty."""
    d2 = [BASE] + ([flipped(BASE, 11, 100)] if second_choice else [])
    d1 = [flipped(BASE, 2, 0), flipped(BASE, 1, 100)]
    return bow_case(d1, {4: [0, 1]}, d2, {4: list(range(len(d2)))})


def bow_disjoint_case():
    """Node lists 1 2 3 10 20 / 5 10 15 20 25: the walk jumps on KF1's side (1 -> 10), on KF2's (5 -> 10),
    matches 10, jumps on KF2's side (15 -> 20) and matches 20.  One identical pair per node."""
    rng = np.random.default_rng(3)
    d = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    return bow_case(d, {1: [0], 2: [1], 3: [2], 10: [3], 20: [4]}, d, {5: [0], 10: [3], 15: [1], 20: [4], 25: [2]})


def bow_live_case(side):
    c = bow_case([BASE, flipped(BASE, 3)], {3: [0, 1]}, [BASE, flipped(BASE, 3)], {3: [0, 1]})
    if side:
        c["live" + side][0] = 0
    return c


def bow_orientation_case(ori):
    """Twelve identical pairs turned by 10 degrees and one turned by 180: its bin holds 1 < 0.1 * 12."""
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, (13, 32), dtype=np.uint8)
    a1 = np.full(13, 100, f32)
    a2 = np.full(13, 90, f32)
    a2[6] = 280
    return bow_case(d, {9: list(range(13))}, d, {9: list(range(13))[::-1]}, a1, a2, ori=ori)


def bow_shape_case(n1n, n2n, seed=5):
    """One big shared node (plus a one-entry node): every KF1 keypoint has its own copy at distance 4 in the
    node's KF2 list when n2n >= n1n, else the later ones find theirs taken."""
    rng = np.random.default_rng(seed)
    n1, n2 = n1n + 1, n2n + 1
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    tgt = np.arange(n1) % n2n
    tgt[-1] = n2 - 1
    d1 = np.array([flipped(d2[t], 4, 9) for t in tgt])
    fv1 = {9: [int(i) for i in rng.permutation(n1n)], 12: [n1 - 1]}
    fv2 = {9: [int(i) for i in rng.permutation(n2n)], 12: [n2 - 1]}
    return bow_case(d1, fv1, d2, fv2, rng.uniform(0, 360, n1), rng.uniform(0, 360, n2), ori=True)


BOW_CRAFTED = [bow_threshold_case(49), bow_threshold_case(50), bow_ratio_case(45, 50), bow_ratio_case(44, 50),
               bow_tie_case([0, 1, 2]), bow_tie_case([2, 0, 1]), bow_tie_case([1, 2, 0]), bow_taken_case(True),
               bow_taken_case(False), bow_disjoint_case(), bow_live_case(None), bow_live_case("1"),
               bow_live_case("2"), bow_orientation_case(True), bow_orientation_case(False)]


# ---------------------------------------------------------------- CPU: the BoW restatement
@pytest.mark.parametrize("i", range(len(BOW_GENERAL)))
def test_bow_restatement_matches_python(i):
    c, (n, m, codes) = bow_general_cached(i)
    ne, me = py_bow(c)
    assert n == ne and np.array_equal(m, me)
    assert n >= 20, n
    assert n == int((m >= 0).sum()) == int((codes == BOW_ACCEPTED).sum())
    # vbMatched2: no KF2 keypoint is given twice
    assert len(set(m[m >= 0].tolist())) == n
    # both lower_bound jumps are taken: each side has private node ids between shared ones
    s1, s2 = set(c["fv1"]), set(c["fv2"])
    assert any(min(s2) < x < max(s2) for x in s1 - s2) and any(min(s1) < x < max(s1) for x in s2 - s1)


def test_bow_general_sequential_dependency_is_reached():
    """Without vbMatched2 some KF2 keypoint would be given twice: the general cases do reach :884."""
    c = bow_general_cached(1)[0]
    twice = 0
    for node, l1 in c["fv1"].items():
        l2 = [j for j in c["fv2"].get(node, []) if c["live2"][j]]
        best = {}
        for i1 in l1:
            if c["live1"][i1] and l2:
                ds = [hamming(c["desc1"][i1], c["desc2"][j]) for j in l2]
                if min(ds) < 50:
                    best.setdefault(l2[int(np.argmin(ds))], []).append(i1)
        twice += sum(len(v) > 1 for v in best.values())
    assert twice >= 5


def test_bow_crafted_cases_take_their_branch():
    seen = set()
    for c in BOW_CRAFTED:
        n, m, codes = ref_bow(c)
        assert (n, m.tolist()) == (py_bow(c)[0], py_bow(c)[1].tolist())
        seen |= set(codes.tolist())
    assert seen == ALL_BOW_CODES, sorted(ALL_BOW_CODES - seen)
    # TH_LOW is strict here: 49 passes, 50 does not; a single candidate leaves bestDist2 = 256
    assert ref_bow(bow_threshold_case(49))[2].tolist() == [BOW_ACCEPTED]
    assert ref_bow(bow_threshold_case(50))[2].tolist() == [BOW_TH_LOW]
    # 45 < 0.9f * 50 = 45.0f is false, 44 < 45.0f is true
    assert f32(0.9) * f32(50) == f32(45)
    assert ref_bow(bow_ratio_case(45, 50))[2].tolist() == [RATIO]
    n, m, codes = ref_bow(bow_ratio_case(44, 50))
    assert codes.tolist() == [BOW_ACCEPTED] and m.tolist() == [1]
    # a single candidate passes any ratio below 1: 49 < 0.6 * 256
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        assert ref_bow(bow_tie_case(order))[1].tolist() == [order[0]]
    n, m, codes = ref_bow(bow_taken_case(True))
    assert m.tolist() == [0, 1] and codes.tolist() == [BOW_ACCEPTED, BOW_ACCEPTED]
    c = bow_taken_case(True)
    assert hamming(c["desc1"][1], c["desc2"][0]) < hamming(c["desc1"][1], c["desc2"][1])  # its second choice
    n, m, codes = ref_bow(bow_taken_case(False))
    assert m.tolist() == [0, -1] and codes.tolist() == [BOW_ACCEPTED, BOW_NO_CANDIDATE]
    n, m, codes = ref_bow(bow_disjoint_case())
    assert m.tolist() == [-1, -1, -1, 3, 4] and codes[:3].tolist() == [NO_SHARED_NODE] * 3
    assert ref_bow(bow_live_case(None))[1].tolist() == [0, 1]
    n, m, codes = ref_bow(bow_live_case("1"))
    assert m.tolist() == [-1, 1] and codes[0] == NOT_LIVE
    n, m, codes = ref_bow(bow_live_case("2"))  # KF1 #0 falls to KF2 #1 (distance 3), KF1 #1 finds nothing left
    assert m.tolist() == [1, -1] and codes.tolist() == [BOW_ACCEPTED, BOW_NO_CANDIDATE]
    n, m, codes = ref_bow(bow_orientation_case(True))
    assert n == 12 and m[6] == -1 and codes[6] == HISTOGRAM
    n, m, codes = ref_bow(bow_orientation_case(False))
    assert n == 13 and m[6] == 6
    for n1n, n2n in ((1, 1), (70, 70), (300, 300)):
        c = bow_shape_case(n1n, n2n)
        c["ori"] = False
        n, m, codes = ref_bow(c)
        assert n == n1n + 1 and set(codes.tolist()) == {BOW_ACCEPTED}


# ====================================================================== SearchByProjection(pKF, Scw, ...)
LOOP_CALLS = [(8, 1.5, 1), (5, 1.0, 0), (3, 1.5, 0)]  # (th, ratioHamming, projection): LoopClosing.cc:929, :954, :1207


def sim3_general(seed, n_kp=300, n_pt=240):
    """util.reloc_case read as (keyframe, candidate points): the same tables, plus the viewing-angle dot
    product on both sides of 0.5 * dist."""
    c = util.reloc_case(seed, n_cur=n_kp, n_kf=n_pt, pre_blocked=0.2)
    rng = np.random.default_rng(seed + 1000)
    c["dot"] = (c["dist"][:, 0].astype(np.float64) * rng.uniform(0.35, 1.0, n_pt))
    return c


def sim3_params(c, th, ratio, projection):
    p = plvi.Sim3ProjParams()
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in c["camera"][:4])
    (p.min_x, p.max_x, p.min_y, p.max_y, p.inv_w, p.inv_h) = c["grid"]
    p.th, p.ratio_hamming, p.projection = int(th), float(ratio), int(projection)
    p.nlevels = len(c["scale_factors"])
    for i, s in enumerate(c["scale_factors"]):
        p.scale_factors[i] = s
    return p


def ref_sim3(c, th, ratio, projection):
    """(nmatches, match, codes, uv) of the restatement."""
    n_kp, n_pt = len(c["cur_kps"]), len(c["kf_flags"])
    p = sim3_params(c, th, ratio, projection)
    m = np.full(max(n_kp, 1), -7, np.int32)
    codes = np.zeros(max(n_pt, 1), np.int32)
    uv = np.full((max(n_pt, 1), 2), np.nan, f32)
    arr = {k: np.ascontiguousarray(c[k]) for k in ("cur_kps", "cur_desc", "cur_blocked", "kf_flags", "x3dc", "dist",
                                                    "dot", "level", "mp_desc")}
    assert arr["dot"].dtype == np.float64 and arr["x3dc"].dtype == f32 and arr["level"].dtype == np.int32
    n = ref_lib().loop_ref_sim3_projection(ctypes.byref(p), _p(arr["cur_kps"]), _p(arr["cur_desc"]), n_kp,
                                           _p(arr["cur_blocked"]), _p(arr["kf_flags"]), _p(arr["x3dc"]),
                                           _p(arr["dist"]), _p(arr["dot"]), _p(arr["level"]), _p(arr["mp_desc"]),
                                           n_pt, _p(m), _p(codes), _p(uv))
    return n, m[:n_kp], codes[:n_pt], uv[:n_pt]


def gpu_sim3(c, th, ratio, projection):
    return plvi.ORBmatcher().SearchByProjectionSim3(sim3_params(c, th, ratio, projection), c["cur_kps"], c["cur_desc"],
                                                    c["kf_flags"], c["x3dc"], c["dist"], c["dot"], c["level"],
                                                    c["mp_desc"], c["cur_blocked"], projection)


def check_gpu_sim3(c, th, ratio, projection):
    ne, me, _, _ = ref_sim3(c, th, ratio, projection)
    ng, mg = gpu_sim3(c, th, ratio, projection)
    assert ng == ne and np.array_equal(mg, me)


def _fmaf(a, b, c):
    if hasattr(math, "fma"):
        return f32(math.fma(float(a), float(b), float(c)))
    from fractions import Fraction
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return f32(f32(a) * f32(b) + f32(c))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    lo = f32(float(exact))  # within one float of the answer: pick the nearer neighbour exactly, ties to even
    cands = sorted({float(lo), float(np.nextafter(lo, f32(-np.inf))), float(np.nextafter(lo, f32(np.inf)))})
    best = min(cands, key=lambda x: (abs(Fraction(x) - exact), int(f32(x).view(np.uint32)) & 1))
    return f32(best)


def py_sim3(c, th, ratio, projection):
    """Pure-Python restatement of ORBmatcher.cc:473-586 / :588-704 downstream of the caller's inputs."""
    k = c["cur_kps"]
    n_kp = len(k)
    min_x, max_x, min_y, max_y, inv_w, inv_h = (f32(v) for v in c["grid"])
    cells = [[[] for _ in range(48)] for _ in range(64)]
    for i in range(n_kp):  # AssignFeaturesToGrid / PosInGrid (std::round: half away from zero)
        gx, gy = f32(f32(k["x"][i] - min_x) * inv_w), f32(f32(k["y"][i] - min_y) * inv_h)
        px = int(math.floor(gx + 0.5)) if gx >= 0 else -int(math.floor(-gx + 0.5))
        py = int(math.floor(gy + 0.5)) if gy >= 0 else -int(math.floor(-gy + 0.5))
        if 0 <= px < 64 and 0 <= py < 48:
            cells[px][py].append(i)
    fx, fy, cx, cy = (f32(v) for v in c["camera"][:4])
    sf = c["scale_factors"]
    matched = c["cur_blocked"].astype(bool).copy()
    out = np.full(n_kp, -1, np.int32)
    nm = 0
    thr = f32(50) * f32(ratio)
    with np.errstate(all="ignore"):
        for i in range(len(c["kf_flags"])):
            if not c["kf_flags"][i] & 1:
                continue
            X, Y, Z = (f32(t) for t in c["x3dc"][i])
            if Z < 0:
                continue
            if projection:
                invz = f32(f32(1) / Z)
                u, v = _fmaf(f32(X * invz), fx, cx), _fmaf(f32(Y * invz), fy, cy)
            else:
                u, v = f32(f32(f32(fx * X) / Z) + cx), f32(f32(f32(fy * Y) / Z) + cy)
            if not (u >= min_x and u < max_x and v >= min_y and v < max_y):
                continue
            d3, dmin, dmax = (f32(t) for t in c["dist"][i])
            if d3 < dmin or d3 > dmax:
                continue
            if float(c["dot"][i]) < 0.5 * float(d3):
                continue
            L = int(c["level"][i])
            if L < 0 or L >= len(sf):
                continue
            r = f32(f32(th) * f32(sf[L]))
            x0 = max(0, math.floor(f32(f32(f32(u - min_x) - r) * inv_w)))
            x1 = min(63, math.ceil(f32(f32(f32(u - min_x) + r) * inv_w)))
            y0 = max(0, math.floor(f32(f32(f32(v - min_y) - r) * inv_h)))
            y1 = min(47, math.ceil(f32(f32(f32(v - min_y) + r) * inv_h)))
            if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
                continue
            best, bi = 256, -1
            for ix in range(x0, x1 + 1):
                for iy in range(y0, y1 + 1):
                    for i2 in cells[ix][iy]:
                        if not (abs(f32(k["x"][i2] - u)) < r and abs(f32(k["y"][i2] - v)) < r):
                            continue
                        if matched[i2]:
                            continue
                        o = int(k["octave"][i2])
                        if o < L - 1 or o > L:
                            continue
                        d = hamming(c["mp_desc"][i], c["cur_desc"][i2])
                        if d < best:
                            best, bi = d, i2
            if f32(best) <= thr:
                out[bi] = i
                matched[bi] = True
                nm += 1
    return nm, out


# crafted cases: unit camera, z = 1
UNIT_CAM = (f32(1), f32(1), f32(0), f32(0), f32(0))
PT_DESC = np.arange(32, dtype=np.uint8) * 11


def kpt(x, y, octave=0):
    k = np.zeros(1, plvi.KEYPOINT_DTYPE)[0]
    k["x"], k["y"], k["octave"], k["size"], k["class_id"] = x, y, octave, 31.0, -1
    return k


def pt(u, v, desc=PT_DESC, level=0, flag=1, z=1.0, dist=(5.0, 2.5, 10.0), dot=5.0):
    return dict(u=u, v=v, desc=desc, level=level, flag=flag, z=z, dist=dist, dot=dot)


def sim3_case(kps, descs, pts, matched=None):
    n, m = len(kps), len(pts)
    z = np.array([q["z"] for q in pts], np.float64).reshape(m)
    x3 = np.stack([np.array([q["u"] for q in pts], np.float64).reshape(m) * z,
                   np.array([q["v"] for q in pts], np.float64).reshape(m) * z, z], 1).astype(f32).reshape(m, 3)
    return {"cur_kps": np.array(kps, plvi.KEYPOINT_DTYPE).reshape(n),
            "cur_desc": np.array(descs, np.uint8).reshape(n, 32),
            "cur_blocked": np.zeros(n, np.uint8) if matched is None else np.asarray(matched, np.uint8),
            "grid": plvi.grid_geometry(752, 480), "scale_factors": util.orb_scale_factors(), "camera": UNIT_CAM,
            "x3dc": x3, "dist": np.array([q["dist"] for q in pts], f32).reshape(m, 3),
            "dot": np.array([q["dot"] for q in pts], np.float64).reshape(m),
            "level": np.array([q["level"] for q in pts], np.int32).reshape(m),
            "kf_flags": np.array([q["flag"] for q in pts], np.uint8).reshape(m),
            "mp_desc": np.array([q["desc"] for q in pts], np.uint8).reshape(m, 32)}


def one_point(**kw):
    """One point at (100, 100) with its own descriptor on a keypoint two pixels away."""
    return sim3_case([kpt(102, 99)], [PT_DESC], [pt(100.0, 100.0, **kw)])


def rejection_cases():
    """(name, case, expected code of point 0) at th 5 / ratio 1.0 / either projection."""
    far = sim3_case([kpt(300, 300)], [PT_DESC], [pt(100.0, 100.0)])
    other_level = sim3_case([kpt(102, 99, 3)], [PT_DESC], [pt(100.0, 100.0, level=1)])
    entry = sim3_case([kpt(102, 99)], [PT_DESC], [pt(100.0, 100.0)], matched=[1])
    over = sim3_case([kpt(102, 99)], [flipped(PT_DESC, 51)], [pt(100.0, 100.0)])
    edge = lambda u, v: sim3_case([kpt(u, v)], [PT_DESC], [pt(u, v)])  # noqa: E731
    return [("accepted", one_point(), ACCEPTED), ("flag", one_point(flag=0), FLAG), ("depth", one_point(z=-1.0), DEPTH),
            ("z=0", one_point(z=0.0), IMAGE), ("left of the image", edge(-1.0, 100.0), IMAGE),
            ("u == min_x", edge(0.0, 100.0), ACCEPTED), ("u == max_x", edge(752.0, 100.0), IMAGE),
            ("v == min_y", edge(100.0, 0.0), ACCEPTED), ("v == max_y", edge(100.0, 480.0), IMAGE),
            # (the last grid column ends before max_x: just below it the point is in the image, without keypoints)
            ("below max_x", sim3_case([kpt(300, 300)], [PT_DESC], [pt(float(np.nextafter(f32(752), f32(0))), 100.0)]),
             EMPTY_WINDOW),
            ("too near", one_point(dist=(2.0, 2.5, 10.0)), DISTANCE),
            ("too far", one_point(dist=(11.0, 2.5, 10.0)), DISTANCE),
            ("dist == min", one_point(dist=(2.5, 2.5, 10.0), dot=2.0), ACCEPTED),
            ("dist == max", one_point(dist=(10.0, 2.5, 10.0)), ACCEPTED),
            ("angle", one_point(dot=float(np.nextafter(2.5, 0.0))), ANGLE),
            ("dot == 0.5 dist", one_point(dot=2.5), ACCEPTED),
            ("level -1", one_point(level=-1), LEVEL),
            ("level == nlevels", one_point(level=len(util.orb_scale_factors())), LEVEL),
            ("empty window", far, EMPTY_WINDOW), ("other level", other_level, NO_CANDIDATE),
            ("matched on entry", entry, NO_CANDIDATE), ("over the threshold", over, THRESHOLD)]


def level_case(L):
    """Keypoints of octaves 0..4 around the point, distances 0, 1, 2, 3, 4: the best octave in [L-1, L] wins."""
    kps = [kpt(100 + o, 100, o) for o in range(5)]
    return sim3_case(kps, [flipped(PT_DESC, o) for o in range(5)], [pt(100.0, 100.0, level=L)])


def threshold_case(nbits):
    return sim3_case([kpt(101, 100)], [flipped(PT_DESC, nbits)], [pt(100.0, 100.0)])


def contention_case(second_dist):
    """Three points with one descriptor on one spot, keypoint A at distance 0 and B at `second_dist`: the
    first takes A, the second is re-scanned and falls to B, the third has none left."""
    return sim3_case([kpt(101, 100), kpt(99, 101)], [PT_DESC, flipped(PT_DESC, second_dist)],
                     [pt(100.0, 100.0), pt(100.0, 100.0), pt(100.0, 100.0)])


def entry_matched_case():
    """A (distance 0) is matched on entry: the point takes B (distance 9), A's row stays -1."""
    return sim3_case([kpt(101, 100), kpt(99, 101)], [PT_DESC, flipped(PT_DESC, 9)], [pt(100.0, 100.0)], matched=[1, 0])


def projection_split_case():
    """An input on which the two projection forms differ in the bits of u and in the result: u of form 0 is
    just inside the window of a keypoint, u of form 1 is not (or the reverse).  Searched with the
    restatement; None when the search finds nothing."""
    if "split" in _cache:
        return _cache["split"]
    rng = np.random.default_rng(77)
    base = sim3_general(7, 4, 1)
    base["cur_blocked"][:] = 0
    base["kf_flags"][:] = 1
    base["level"][:] = 0
    base["dist"][:] = (5.0, 2.5, 10.0)
    base["dot"][:] = 5.0
    base["cur_kps"]["octave"] = 0
    base["cur_kps"]["x"], base["cur_kps"]["y"] = 5.0, 5.0
    base["cur_desc"][:] = base["mp_desc"][0]
    found = None
    for _ in range(4000):
        z = rng.uniform(1, 20)
        u0, v0 = rng.uniform(50, 700), rng.uniform(50, 430)
        fx, fy, cx, cy = (float(t) for t in base["camera"][:4])
        base["x3dc"][0] = ((u0 - cx) * z / fx, (v0 - cy) * z / fy, z)
        ua = ref_sim3(base, 5, 1.0, 0)[3][0]
        ub = ref_sim3(base, 5, 1.0, 1)[3][0]
        if ua[0] == ub[0]:
            continue
        lo = min(ua[0], ub[0])
        for step in range(-3, 4):  # a keypoint whose |dx| < 5 holds for one u only
            kx = f32(lo + f32(5))
            for _ in range(abs(step)):
                kx = np.nextafter(kx, f32(np.inf if step > 0 else -np.inf))
            base["cur_kps"]["x"][0], base["cur_kps"]["y"][0] = kx, ua[1]
            ra, rb = ref_sim3(base, 5, 1.0, 0), ref_sim3(base, 5, 1.0, 1)
            if ra[0] != rb[0]:
                found = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in base.items()}
                break
        if found:
            break
    _cache["split"] = found
    return found


SIM3_GENERAL = [11, 12, 13]


def sim3_general_cached(seed, n_kp=300, n_pt=240):
    key = ("sim3", seed, n_kp, n_pt)
    if key not in _cache:
        c = sim3_general(seed, n_kp, n_pt)
        _cache[key] = (c, {call: ref_sim3(c, *call) for call in LOOP_CALLS})
    return _cache[key]


# ---------------------------------------------------------------- CPU: the projection restatement
@pytest.mark.parametrize("seed", SIM3_GENERAL)
@pytest.mark.parametrize("call", LOOP_CALLS, ids=["th8-r1.5-kfs", "th5-r1.0", "th3-r1.5"])
def test_sim3_restatement_matches_python(seed, call):
    c, refs = sim3_general_cached(seed)
    n, m, codes, _ = refs[call]
    ne, me = py_sim3(c, *call)
    assert n == ne and np.array_equal(m, me)
    assert n >= 20, n
    assert n == int((m >= 0).sum()) == int((codes == ACCEPTED).sum())
    assert (m[c["cur_blocked"] == 1] == -1).all()  # matched on entry: never overwritten
    assert len(set(m[m >= 0].tolist())) == n
    # the other projection form on the same input, against Python as well
    other = (call[0], call[1], 1 - call[2])
    no, mo, _, _ = ref_sim3(c, *other)
    npy, mpy = py_sim3(c, *other)
    assert no == npy and np.array_equal(mo, mpy)


def test_sim3_general_sequential_dependency_is_reached():
    """Walking the points in the opposite order assigns differently: phase 2 matters on the general case."""
    c, refs = sim3_general_cached(SIM3_GENERAL[0])
    rev = dict(c)
    for k in ("kf_flags", "x3dc", "dist", "dot", "level", "mp_desc"):
        rev[k] = c[k][::-1].copy()
    mr = ref_sim3(rev, 8, 1.5, 1)[1]
    n_pt = len(c["kf_flags"])
    assert not np.array_equal(np.where(mr >= 0, n_pt - 1 - mr, mr), refs[(8, 1.5, 1)][1])


def test_sim3_crafted_cases_take_their_branch():
    seen = set()
    for name, c, code in rejection_cases():
        for projection in (0, 1):
            n, m, codes, uv = ref_sim3(c, 5, 1.0, projection)
            assert codes[0] == code, (name, projection, codes[0])
            assert n == (code == ACCEPTED) and (n, m.tolist()) == (py_sim3(c, 5, 1.0, projection)[0],
                                                                   py_sim3(c, 5, 1.0, projection)[1].tolist()), name
            seen.add(int(codes[0]))
    assert seen == ALL_SIM3_CODES, sorted(ALL_SIM3_CODES - seen)
    # octave in [L-1, L]: the lowest admissible octave has the smallest distance
    for L, want in ((0, 0), (1, 0), (2, 1), (3, 2), (4, 3), (5, 4)):
        assert ref_sim3(level_case(L), 8, 1.0, 0)[1].tolist() == [0 if o == want else -1 for o in range(5)], L
    n, m, codes, _ = ref_sim3(level_case(6), 8, 1.0, 0)
    assert n == 0 and codes[0] == NO_CANDIDATE
    # bestDist <= TH_LOW * ratioHamming with loop closing's three (th, ratio) pairs
    for th, ratio, projection in LOOP_CALLS:
        edge = 75 if ratio == 1.5 else 50
        assert ref_sim3(threshold_case(edge), th, ratio, projection)[2].tolist() == [ACCEPTED]
        assert ref_sim3(threshold_case(edge + 1), th, ratio, projection)[2].tolist() == [THRESHOLD]
    n, m, codes, _ = ref_sim3(contention_case(10), 5, 1.0, 0)
    assert m.tolist() == [0, 1] and codes.tolist() == [ACCEPTED, ACCEPTED, NO_CANDIDATE]
    n, m, codes, _ = ref_sim3(contention_case(60), 5, 1.0, 0)  # the re-scanned best is over the threshold
    assert m.tolist() == [0, -1] and codes.tolist() == [ACCEPTED, THRESHOLD, THRESHOLD]
    assert ref_sim3(contention_case(60), 5, 1.5, 0)[1].tolist() == [0, 1]
    n, m, codes, _ = ref_sim3(entry_matched_case(), 5, 1.0, 0)
    assert m.tolist() == [-1, 0] and codes.tolist() == [ACCEPTED]


def test_projection_forms_differ():
    """The :588 overload is not an alias of the :473 one: an input whose u differs in the last bit between
    (fx*x)/z + cx and fma(x * (1/z), fx, cx), with a keypoint inside the window of one form only."""
    c = projection_split_case()
    assert c is not None
    ra, rb = ref_sim3(c, 5, 1.0, 0), ref_sim3(c, 5, 1.0, 1)
    assert ra[3][0][0] != rb[3][0][0] and abs(float(ra[3][0][0]) - float(rb[3][0][0])) < 1e-3
    assert {ra[0], rb[0]} == {0, 1} and {int(ra[2][0]), int(rb[2][0])} == {ACCEPTED, EMPTY_WINDOW}
    for projection, r in ((0, ra), (1, rb)):
        npy, mpy = py_sim3(c, 5, 1.0, projection)
        assert npy == r[0] and np.array_equal(mpy, r[1])


# ====================================================================== GPU
@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(BOW_GENERAL)))
def test_gpu_bow_general_parity(plvi_lib, i):
    c, (ne, me, _) = bow_general_cached(i)
    ng, mg = gpu_bow(c)
    assert ng == ne and np.array_equal(mg, me)
    big = bow_general(50 + i, 1100 - 300 * i, 500 + 300 * i, ori=bool(i & 1), nnratio=0.75)
    check_gpu_bow(big)


@pytest.mark.gpu
def test_gpu_bow_crafted(plvi_lib):
    for c in BOW_CRAFTED:
        check_gpu_bow(c)


@pytest.mark.gpu
def test_gpu_bow_launch_shapes(plvi_lib):
    # nodes of 1, of more than a wave, longer than the 256-thread strides; fewer KF2 entries than KF1 entries
    for n1n, n2n in ((1, 1), (70, 70), (300, 300), (3, 300), (300, 3), (130, 65)):
        check_gpu_bow(bow_shape_case(n1n, n2n))
    c = bow_shape_case(5, 5)
    e = dict(c, desc1=c["desc1"][:0], angle1=c["angle1"][:0], live1=c["live1"][:0], fv1={})  # n1 = 0
    n, m = gpu_bow(e)
    assert n == 0 and len(m) == 0
    e = dict(c, desc2=c["desc2"][:0], angle2=c["angle2"][:0], live2=c["live2"][:0], fv2={})  # n2 = 0
    n, m = gpu_bow(e)
    assert n == 0 and np.array_equal(m, np.full(6, -1))
    e = dict(c, live2=np.zeros(6, np.uint8))
    check_gpu_bow(e)


def _bow_tuple(c):
    """The case in tests/batch_pack.py's SearchByBoW layout (KF side = KF1, F side = KF2)."""
    return (c["desc1"], c["angle1"], c["live1"], c["fv1"], c["desc2"], c["angle2"], c["fv2"])


# the keys of the packed tables in the header's order (batch_pack.pack_bow names: k* = KF1, f* = KF2)
BOW_KF1_KEYS = ("kd", "ka", "kl", "d_n1", "kn", "ko", "d_nn1", "ki")
BOW_KF2_KEYS = ("fd", "fa", "fl", "d_n2", "fn", "fo", "d_nn2", "fi")


def _bow_batch(over=True):
    sizes = [(96, 96), (40, 80), (77, 1), (64, 50)]
    cases = [bow_general(60 + i, a, b, ori=True) for i, (a, b) in enumerate(sizes)]
    cap1 = cap2 = 96
    node_cap = max(max(len(c["fv1"]), len(c["fv2"])) for c in cases)
    b = bp.pack_bow([_bow_tuple(c) for c in cases], cap1, cap2, node_cap)
    b["fl"] = bp.pack_rows([c["live2"] for c in cases], cap2, [np.ones(1, np.uint8)] * len(cases))
    # pair 0 fills the tables: its counts are given above the capacities and must read as clamped
    ov = {0: 1} if over else {}
    b["d_n1"] = bp.counts_array(b["kf_n"], {p: cap1 + 5 for p in ov})
    # pair 2: a negative count reads as 0
    b["d_n2"] = bp.counts_array(b["f_n"], {**{p: cap2 + 1000 for p in ov}, 2: -1})
    b["d_nn1"] = bp.counts_array(b["kc"], {p: node_cap + 3 for p in ov if b["kc"][p] == node_cap})
    b["d_nn2"] = bp.counts_array(b["fc"], {p: node_cap + 1 for p in ov if b["fc"][p] == node_cap})
    return cases, b, cap1, cap2, node_cap


@pytest.mark.gpu
def test_gpu_bow_batch_of_four(plvi_lib):
    cases, b, cap1, cap2, node_cap = _bow_batch()
    P = len(cases)
    dev = bp.Device()
    out, get_m = dev.canary(P + bp.SLACK, cap1)
    cnt, get_n = dev.canary(P + bp.SLACK)
    kf1 = [dev.up(b[k]).value for k in BOW_KF1_KEYS]
    kf2 = [dev.up(b[k]).value for k in BOW_KF2_KEYS]
    plvi.search_by_bow_kf_batch(P, 0.75, True, cap1, cap2, node_cap, kf1, kf2, out.value, cnt.value)
    cases[2] = dict(cases[2], desc2=cases[2]["desc2"][:0], angle2=cases[2]["angle2"][:0], live2=cases[2]["live2"][:0],
                    fv2={})
    refs = [ref_bow(c) for c in cases]
    assert sum(r[0] for r in refs) >= 20 and refs[0][0] >= 10 and refs[2][0] == 0
    bp.check_rows(get_m(), [m for _, m, _ in refs], "search_by_bow_kf matches12")
    bp.check_counts(get_n(), [n for n, _, _ in refs], "search_by_bow_kf")
    # the LDS rule: 4 * cap1 + 8 * node_cap + cap2 bytes against 160 KB, refused before any launch
    before = get_m()
    rc = plvi_lib.plvi_search_by_bow_kf_batch(P, 0.75, 1, 41000, cap2, node_cap, *[ctypes.c_void_p(x) for x in kf1],
                                              *[ctypes.c_void_p(x) for x in kf2], out, cnt, None)
    assert rc == plvi.PLVI_E_CAPACITY
    assert np.array_equal(get_m(), before)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SIM3_GENERAL)
def test_gpu_sim3_general_parity(plvi_lib, seed):
    c, refs = sim3_general_cached(seed)
    for call in LOOP_CALLS:
        ne, me = refs[call][:2]
        ng, mg = gpu_sim3(c, *call)
        assert ng == ne and np.array_equal(mg, me), call
    # more than one 256-thread stride on both sides
    big = sim3_general(seed + 20, 1100 - 100 * (seed % 3), 900 - 50 * (seed % 3))
    for call in LOOP_CALLS:
        ne = ref_sim3(big, *call)[0]
        assert ne >= 20
        check_gpu_sim3(big, *call)
        check_gpu_sim3(big, call[0], call[1], 1 - call[2])


@pytest.mark.gpu
def test_gpu_sim3_three_times_as_many_points(plvi_lib):
    c = sim3_general(31, 300, 900)
    assert ref_sim3(c, 8, 1.5, 1)[0] >= 20
    for call in LOOP_CALLS:
        check_gpu_sim3(c, *call)


@pytest.mark.gpu
def test_gpu_sim3_crafted(plvi_lib):
    for name, c, _ in rejection_cases():
        for projection in (0, 1):
            check_gpu_sim3(c, 5, 1.0, projection)
    for L in range(7):
        check_gpu_sim3(level_case(L), 8, 1.0, 0)
    for th, ratio, projection in LOOP_CALLS:
        edge = 75 if ratio == 1.5 else 50
        check_gpu_sim3(threshold_case(edge), th, ratio, projection)
        check_gpu_sim3(threshold_case(edge + 1), th, ratio, projection)
    for projection in (0, 1):
        check_gpu_sim3(contention_case(10), 5, 1.0, projection)
        check_gpu_sim3(contention_case(60), 5, 1.0, projection)
        check_gpu_sim3(contention_case(60), 5, 1.5, projection)
        check_gpu_sim3(entry_matched_case(), 5, 1.0, projection)
    c = projection_split_case()
    assert c is not None
    check_gpu_sim3(c, 5, 1.0, 0)
    check_gpu_sim3(c, 5, 1.0, 1)


PT_KEYS = ("kf_flags", "x3dc", "dist", "dot", "level", "mp_desc")


@pytest.mark.gpu
def test_gpu_sim3_degenerate(plvi_lib):
    case = sim3_general(9, 60, 5)
    for n_pt in (0, 1, 5):
        c = dict(case)
        for key in PT_KEYS:
            c[key] = case[key][:n_pt]
        for blk in (case["cur_blocked"], np.ones(60, np.uint8)):  # all keypoints matched on entry
            c["cur_blocked"] = blk
            check_gpu_sim3(c, 8, 1.5, 1)
    c = dict(case)  # no keypoints
    c["cur_kps"], c["cur_desc"], c["cur_blocked"] = case["cur_kps"][:0], case["cur_desc"][:0], case["cur_blocked"][:0]
    n, m = gpu_sim3(c, 8, 1.5, 0)
    assert n == 0 and len(m) == 0
    with pytest.raises(RuntimeError):  # 50 * 5.12 = 256: a search without a candidate would index vpMatched[-1]
        gpu_sim3(case, 8, 5.12, 0)
    check_gpu_sim3(case, 8, 5.0, 0)


def _sim3_poison(c):
    """Padding rows of the point tables: aimed exactly at keypoints the true answer leaves alone, with those
    keypoints' own descriptor, in range and in view."""
    a = bp._aimed(c, "cur_kps", "cur_desc", bp.free_keypoints(c))
    n = len(a["octave"])
    return {"kf_flags": np.ones(n, np.uint8), "x3dc": a["x3dc"], "level": a["octave"], "mp_desc": a["mp_desc"],
            "dist": np.tile(np.array([5.0, 2.5, 10.0], f32), (n, 1)), "dot": np.full(n, 5.0, np.float64)}


SIM3_PT = bp._spec(_sim3_poison, PT_KEYS)


@pytest.mark.gpu
def test_gpu_sim3_batch_of_four(plvi_lib):
    kc, pc = 700, 640
    sizes = [(kc, pc), (520, 240), (300, 600), (410, 1)]
    cases = [sim3_general(80 + i, a, b) for i, (a, b) in enumerate(sizes)]
    P = len(cases)
    b = {**bp.pack_keyed(cases, kc, bp.CUR), **bp.pack_keyed(cases, pc, SIM3_PT)}
    dev = bp.Device()
    dk = dev.up(b["cur_kps"])
    # pair 0 fills both tables: its counts are given above the capacities and must read as clamped
    dn = dev.up(bp.counts_array([len(c["cur_kps"]) for c in cases], {0: kc + 7}))
    dpn = dev.up(bp.counts_array([len(c["kf_flags"]) for c in cases], {0: pc + 1000, 3: -2}))  # pair 3: reads as 0
    off, idx = bp.assign_grid(dev, dk, dn, kc, P, cases[0]["grid"], [c["cur_kps"] for c in cases])
    # the packed cur_blocked padding is 0 (free): the real rows carry each case's flags
    kf = [dk.value, dev.up(b["cur_desc"]).value, dn.value, dev.up(b["cur_blocked"]).value, off.value, idx.value]
    pts = [dev.up(b[k]).value for k in PT_KEYS] + [dpn.value]
    for call in LOOP_CALLS[:2]:
        prm = sim3_params(cases[0], *call)
        out, get_m = dev.canary(P + bp.SLACK, kc)
        nm, get_n = dev.canary(P + bp.SLACK)
        plvi.search_sim3_projection_batch(P, prm, kf, kc, pts, pc, out.value, nm.value)
        no_points = {**cases[3], **{k: cases[3][k][:0] for k in PT_KEYS}}
        refs = [ref_sim3(c, *call) for c in cases[:3]] + [ref_sim3(no_points, *call)]
        assert refs[0][0] >= 20 and refs[1][0] >= 20 and refs[3][0] == 0
        bp.check_rows(get_m(), [r[1] for r in refs], "search_sim3_projection match")
        bp.check_counts(get_n(), [r[0] for r in refs], "search_sim3_projection")
    # the LDS rule: 17 * kp_cap + 4 * pt_cap + 12292 + 64 bytes against 160 KB, refused before any launch
    before = get_m()
    V = ctypes.c_void_p
    args = [V(x) for x in kf[:2]] + [V(kf[2]), kc] + [V(x) for x in kf[3:]] + [V(x) for x in pts[:6]] + [V(pts[6])]
    rc = plvi_lib.plvi_search_sim3_projection_batch(P, ctypes.byref(prm), *args, 40000, out, nm, None)
    assert rc == plvi.PLVI_E_CAPACITY
    prm.ratio_hamming = 5.12
    rc = plvi_lib.plvi_search_sim3_projection_batch(P, ctypes.byref(prm), *args, pc, out, nm, None)
    assert rc == plvi.PLVI_E_BADARG
    assert np.array_equal(get_m(), before)
