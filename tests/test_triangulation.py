"""Triangulation-candidate search for new keyframes, points and lines:
ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:965-1206, single-camera
Pinhole branch) and LineMatcher::SearchForTriangulation
(src/LineMatcher.cpp:142-171).

The expected values come from tests/native/triangulation_ref.cpp, a
sequential host restatement built here with -ffp-contract=off.  It also
returns, per KF1 keypoint, why the keypoint ended as it did (the TRI_* codes
below), so every case proves from the restatement alone that its input takes
the branch it is about; the gpu tests then compare the HIP result with the
restatement exactly (matches12 and nmatches; pairs, count and MAD for lines).

Inputs are built by hand: keypoints are projections of random 3-D points
through two float32 poses (so true pairs satisfy the constraint), descriptors
are random 256-bit rows with planted copies at chosen Hamming distances, node
ids are assigned directly, and F12 / the epipole -- inputs of the entry
point -- are computed with numpy.  The crafted cases use F12 = [t]x with
t = (1, 0, 0): the epipolar line of (x1, y1) is y = y1, den = 1 and
dsqr = (y2 - y1)^2, all exact in float.
"""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "triangulation_ref.cpp"
SO = ROOT / "tests" / "native" / "_build" / "libtriangulation_ref.so"

HAS_POINT, STEREO_FILTERED, NO_SHARED_NODE, NO_CANDIDATE, EPIPOLE, EPILINE, ACCEPTED, HISTOGRAM = range(1, 9)
ALL_CODES = set(range(1, 9))

# plvi_triangulation_pair: 9 + 2 floats, two (count, 16 floats) tables, three flags
assert ctypes.sizeof(plvi.TriangulationPair) == 4 * (9 + 2 + 2 * 17 + 3)

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
        V, I = ctypes.c_void_p, ctypes.c_int
        lib.tri_ref_points.argtypes = [V, V, V, I, V, V, I, V, V, V, V, V, I, V, V, I, V, V, V, V, V]
        lib.tri_ref_points.restype = I
        lib.tri_ref_lines.argtypes = [V, I, V, I, V, V, ctypes.c_double, V, V]
        lib.tri_ref_lines.restype = I
        _ref = lib
    return _ref


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------ cases
SCALE = [np.float32(1.2) ** np.float32(i) for i in range(8)]
SIGMA2 = [s * s for s in SCALE]
FX = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)  # [t]x, t = (1, 0, 0)
FAR = (-1000.0, -1000.0)  # an epipole no keypoint is near


def kp(x, y, octave=0, angle=0.0):
    k = np.zeros(1, plvi.KEYPOINT_DTYPE)[0]
    k["x"], k["y"], k["octave"], k["angle"], k["size"] = x, y, octave, angle, 31.0
    return k


def flipped(desc, nbits, start=0):
    """A copy of the 32-byte row with bits [start, start + nbits) flipped."""
    bits = np.unpackbits(desc)
    bits[start:start + nbits] ^= 1
    return np.packbits(bits)


def make_case(kps1, desc1, fv1, kps2, desc2, fv2, F12=FX, ep=FAR, has1=None, ur1=None, has2=None, ur2=None,
              only_stereo=False, coarse=False, ori=False):
    n1, n2 = len(kps1), len(kps2)
    c = dict(kps1=np.array(kps1, plvi.KEYPOINT_DTYPE).reshape(n1), kps2=np.array(kps2, plvi.KEYPOINT_DTYPE).reshape(n2),
             desc1=np.array(desc1, np.uint8).reshape(n1, 32), desc2=np.array(desc2, np.uint8).reshape(n2, 32),
             fv1=fv1, fv2=fv2, F12=np.asarray(F12, np.float32), ep=ep,
             has1=np.zeros(n1, np.uint8) if has1 is None else np.asarray(has1, np.uint8),
             has2=np.zeros(n2, np.uint8) if has2 is None else np.asarray(has2, np.uint8),
             ur1=np.full(n1, -1, np.float32) if ur1 is None else np.asarray(ur1, np.float32),
             ur2=np.full(n2, -1, np.float32) if ur2 is None else np.asarray(ur2, np.float32),
             only_stereo=only_stereo, coarse=coarse, ori=ori)
    return c


def pair_of(c):
    return plvi.TriangulationPair.make(c["F12"], c["ep"], SIGMA2, SCALE, c["only_stereo"], c["coarse"], c["ori"])


def ref_points(c, n1=None, n2=None):
    """(nmatches, matches12, codes) of the restatement."""
    n1 = len(c["kps1"]) if n1 is None else n1
    n2 = len(c["kps2"]) if n2 is None else n2
    a, ao, ai = plvi.feature_vector_csr(c["fv1"])
    b, bo, bi = plvi.feature_vector_csr(c["fv2"])
    pair = pair_of(c)
    m = np.full(max(n1, 1), -7, np.int32)
    codes = np.zeros(max(n1, 1), np.int32)
    n = ref_lib().tri_ref_points(ctypes.byref(pair), _p(c["kps1"]), _p(c["desc1"]), n1, _p(a), _p(ao), len(a), _p(ai),
                                 _p(c["has1"]), _p(c["ur1"]), _p(c["kps2"]), _p(c["desc2"]), n2, _p(b), _p(bo),
                                 len(b), _p(bi), _p(c["has2"]), _p(c["ur2"]), _p(m), _p(codes))
    return n, m[:n1], codes[:n1]


def gpu_points(c):
    """(nmatches, matches12) through the single-pair entry point."""
    n, pairs = plvi.ORBmatcher(0.6, c["ori"]).SearchForTriangulation(
        c["kps1"], c["desc1"], c["fv1"], c["has1"], c["ur1"], c["kps2"], c["desc2"], c["fv2"], c["has2"], c["ur2"],
        c["F12"], c["ep"], SIGMA2, SCALE, c["only_stereo"], c["coarse"])
    m = np.full(len(c["kps1"]), -1, np.int32)
    m[pairs[:, 0]] = pairs[:, 1]
    return n, m


def check_gpu(c):
    ne, me, _ = ref_points(c)
    ng, mg = gpu_points(c)
    assert ng == ne and np.array_equal(mg, me)


def general_case(seed, n1=300, n2=300, ori=True, only_stereo=False):
    """Two views of random 3-D points; ~24 nodes per side, partly disjoint."""
    rng = np.random.default_rng(seed)
    K = np.array([[458.0, 0, 367.0], [0, 457.0, 248.0], [0, 0, 1]])
    ang = 0.05
    R2 = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])  # R2w, camera 1 = world
    t2 = np.array([0.06, 0.02, 0.45])  # forward motion: the epipole lies inside the image
    ntrue = min(200, 2 * min(n1, n2) // 3)
    X = np.stack([rng.uniform(-2, 2, ntrue), rng.uniform(-1.3, 1.3, ntrue), rng.uniform(3, 9, ntrue)], 1)

    def project(Xc):
        u = (K @ Xc.T).T
        return (u[:, :2] / u[:, 2:3]).astype(np.float32)

    uv1, uv2 = project(X), project((R2 @ X.T).T + t2)
    # X1 = R12 X2 + t12 with R12 = R2^T, t12 = -R2^T t2; F12 = K^-T [t12]x R12 K^-1
    R12, t12 = R2.T, -R2.T @ t2
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Kinv = np.linalg.inv(K)
    F12 = (Kinv.T @ tx @ R12 @ Kinv).astype(np.float32)
    e = K @ t2
    ep = (np.float32(e[0] / e[2]), np.float32(e[1] / e[2]))

    k1 = np.zeros(n1, plvi.KEYPOINT_DTYPE)
    k2 = np.zeros(n2, plvi.KEYPOINT_DTYPE)
    k1["x"], k1["y"] = rng.uniform(0, 752, n1), rng.uniform(0, 480, n1)
    k2["x"], k2["y"] = rng.uniform(0, 752, n2), rng.uniform(0, 480, n2)
    k1["octave"], k2["octave"] = rng.integers(0, 8, n1), rng.integers(0, 8, n2)
    k1["angle"], k2["angle"] = rng.uniform(0, 360, n1), rng.uniform(0, 360, n2)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    nodes1 = list(range(100, 100 + 2 * 20, 2)) + [201, 203, 205, 207]  # 24 nodes
    nodes2 = list(range(100, 100 + 2 * 20, 2)) + [131, 133, 300, 301]  # 20 shared, 4 + 4 private
    shared = nodes1[:20]
    node1 = rng.choice(nodes1, n1)
    node2 = rng.choice(nodes2, n2)
    i1s, i2s = rng.permutation(n1)[:ntrue], rng.permutation(n2)[:ntrue]
    free2 = [i for i in range(n2) if i not in set(i2s.tolist())]
    for j, (i1, i2) in enumerate(zip(i1s, i2s)):
        k1["x"][i1], k1["y"][i1] = uv1[j]
        k2["x"][i2], k2["y"][i2] = uv2[j]
        k2["octave"][i2] = rng.integers(0, 3)
        node1[i1] = node2[i2] = rng.choice(shared)
        k1["angle"][i1] = rng.uniform(0, 360)
        # most true pairs turn by about the same angle; one in eight by anything
        k2["angle"][i2] = (k1["angle"][i1] - (rng.uniform(-5, 5) if j % 8 else rng.uniform(0, 360))) % 360
        d1[i1] = flipped(d2[i2], int(rng.integers(0, 62)), int(rng.integers(0, 190)))  # some beyond TH_LOW
        if j % 10 == 0 and j // 10 < len(free2):  # a closer copy off the epipolar line, in the same node
            i2b = free2[j // 10]
            d2[i2b] = flipped(d1[i1], 1, 200)
            node2[i2b] = node2[i2]
            k2["x"][i2b], k2["y"][i2b] = (k2["x"][i2] + 40) % 752, (k2["y"][i2] + 60) % 480
        if j % 10 == 5:  # the true partner sits on the epipole
            k2["x"][i2], k2["y"][i2] = ep[0] + rng.uniform(-3, 3), ep[1] + rng.uniform(-3, 3)
    has1 = (rng.uniform(size=n1) < 0.1).astype(np.uint8)
    has2 = (rng.uniform(size=n2) < 0.1).astype(np.uint8)
    ur1 = np.where(rng.uniform(size=n1) < (0.7 if only_stereo else 0.15), k1["x"] - 20, -1).astype(np.float32)
    ur2 = np.where(rng.uniform(size=n2) < (0.7 if only_stereo else 0.15), k2["x"] - 20, -1).astype(np.float32)
    fv1 = {int(n): [int(i) for i in np.flatnonzero(node1 == n)] for n in nodes1}
    fv2 = {int(n): [int(i) for i in np.flatnonzero(node2 == n)] for n in nodes2}
    fv1[150] = []   # a node with an empty list on either side, shared and private
    fv2[150] = []
    fv1[99] = []
    fv2[400] = []
    for fv in (fv1, fv2):  # FeatureVector order is insertion order, not index order
        for n in fv:
            fv[n] = [int(i) for i in rng.permutation(fv[n])]
    return make_case(k1, d1, fv1, k2, d2, fv2, F12, ep, has1, ur1, has2, ur2, only_stereo, False, ori)


GENERAL = [dict(seed=11, ori=True, only_stereo=False), dict(seed=12, ori=False, only_stereo=False),
           dict(seed=13, ori=True, only_stereo=True)]
_general_cache = {}


def general(i):
    if i not in _general_cache:
        c = general_case(**GENERAL[i])
        _general_cache[i] = (c, ref_points(c))
    return _general_cache[i]


def tie_case(order):
    """KF1 #0 against four KF2 keypoints of one node: #3 at distance 3 but 50 px off the line, listed first;
    #0..#2 at distance 10 (different bits) on the line, listed in `order`."""
    base = np.arange(32, dtype=np.uint8) * 7
    d2 = [flipped(base, 10, 0), flipped(base, 10, 40), flipped(base, 10, 80), flipped(base, 3, 120)]
    k2 = [kp(100, 50), kp(120, 50.5), kp(140, 49.5), kp(160, 100)]
    return make_case([kp(10, 50)], [base], {7: [0]}, k2, d2, {7: [3] + list(order)})


def threshold_case(nbits):
    base = np.arange(32, dtype=np.uint8) * 11
    return make_case([kp(10, 50)], [base], {3: [0]}, [kp(200, 50)], [flipped(base, nbits)], {3: [0]})


def epipole_case(dx, ur1=-1.0, ur2=-1.0, octave=0):
    """The only candidate lies dx to the right of the epipole (0, 50), on KF1 #0's epipolar line: distex = -dx
    and distex^2 are exact or rounded once."""
    base = np.arange(32, dtype=np.uint8) * 13
    return make_case([kp(10, 50)], [base], {3: [0]}, [kp(np.float32(dx), 50, octave)], [base], {3: [0]},
                     ep=(0.0, 50.0), ur1=[ur1], ur2=[ur2])


def stereo_flag_case(only_stereo):
    """Four identical descriptors per side in one node, on one line; #0, #2 of KF1 and #1, #3 of KF2 are stereo."""
    base = np.arange(32, dtype=np.uint8) * 17
    k = [kp(10 + 10 * i, 50) for i in range(4)]
    return make_case(k, [base] * 4, {1: [0, 1, 2, 3]}, k, [base] * 4, {1: [0, 1, 2, 3]}, ur1=[5, -1, 5, -1],
                     ur2=[-1, 5, -1, 5], only_stereo=only_stereo)


def coarse_case(coarse):
    c = stereo_flag_case(False)
    c["F12"] = np.zeros((3, 3), np.float32)
    c["coarse"] = coarse
    return c


def shape_case(n1_in_node, n2_in_node, seed=5):
    """One big shared node (plus a one-entry node): every KF1 keypoint has its copy at distance 4 somewhere in
    the node's KF2 list, on its line."""
    rng = np.random.default_rng(seed)
    n1, n2 = n1_in_node + 1, n2_in_node + 1
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    k2 = [kp(5 + (i % 700), 3 + (i * 7) % 470, i % 3) for i in range(n2)]
    tgt = rng.integers(0, n2_in_node, n1)
    tgt[-1] = n2 - 1
    d1 = [flipped(d2[t], 4, 9) for t in tgt]
    k1 = [kp(700 - (i % 650), k2[t]["y"], 0) for i, t in enumerate(tgt)]
    fv1 = {9: [int(i) for i in rng.permutation(n1_in_node)], 12: [n1 - 1]}
    fv2 = {9: [int(i) for i in rng.permutation(n2_in_node)], 12: [n2 - 1]}
    return make_case(k1, d1, fv1, k2, d2, fv2, ori=True)


def small_case(seed, n1, n2):
    return general_case(seed, n1, n2, ori=bool(seed & 1))


# -------------------------------------------------------- CPU: the restatement
def test_general_cases_reach_every_outcome():
    seen = set()
    for i in range(len(GENERAL)):
        _, (n, m, codes) = general(i)
        assert n == int((m >= 0).sum()) == int((codes == ACCEPTED).sum())
        seen |= set(codes.tolist())
        if not GENERAL[i]["only_stereo"]:
            assert n >= 50, (i, n)
        assert HISTOGRAM not in codes or GENERAL[i]["ori"]
    assert seen == ALL_CODES, sorted(ALL_CODES - seen)
    # both lower_bound jumps of the merge walk are taken: each side has private node ids between shared ones
    c = general(0)[0]
    s1, s2 = set(c["fv1"]), set(c["fv2"])
    assert any(min(s2) < n < max(s2) for n in s1 - s2) and any(min(s1) < n < max(s1) for n in s2 - s1)


def test_tie_rule_last_in_list_order_wins():
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        n, m, codes = ref_points(tie_case(order))
        assert n == 1 and m[0] == order[-1] and codes[0] == ACCEPTED
    # the closer candidate alone: refused by the line test, so it must not have lowered bestDist above
    c = tie_case([])
    n, m, codes = ref_points(c)
    assert n == 0 and codes[0] == EPILINE


def test_many_to_one_keeps_both():
    base = np.arange(32, dtype=np.uint8) * 5
    c = make_case([kp(10, 50), kp(30, 50)], [base, flipped(base, 2)], {4: [0, 1]}, [kp(300, 50), kp(310, 90)],
                  [base, flipped(base, 1)], {4: [0, 1]})
    n, m, codes = ref_points(c)
    assert n == 2 and m.tolist() == [0, 0]


def test_thresholds():
    assert ref_points(threshold_case(50))[0] == 1
    n, _, codes = ref_points(threshold_case(51))
    assert n == 0 and codes[0] == NO_CANDIDATE
    # epipole: 10^2 < 100 * 1 is false (kept), just inside is rejected, just outside kept
    inside, outside = np.nextafter(np.float32(10), np.float32(0)), np.nextafter(np.float32(10), np.float32(20))
    assert ref_points(epipole_case(10.0))[2][0] == ACCEPTED
    assert ref_points(epipole_case(inside))[2][0] == EPIPOLE
    assert ref_points(epipole_case(outside))[2][0] == ACCEPTED
    # the radius grows with the candidate's level: 10 px is inside 10 * sqrt(1.2)
    assert ref_points(epipole_case(10.0, octave=1))[2][0] == EPIPOLE
    # skipped when either side is stereo
    assert ref_points(epipole_case(inside, ur1=3.0))[2][0] == ACCEPTED
    assert ref_points(epipole_case(inside, ur2=0.0))[2][0] == ACCEPTED


def test_flags():
    n, m, codes = ref_points(stereo_flag_case(True))
    assert codes.tolist() == [ACCEPTED, STEREO_FILTERED, ACCEPTED, STEREO_FILTERED] and m.tolist() == [3, -1, 3, -1]
    assert ref_points(stereo_flag_case(False))[1].tolist() == [3, 3, 3, 3]
    n, m, codes = ref_points(coarse_case(False))
    assert n == 0 and set(codes.tolist()) == {EPILINE}  # den == 0 rejects
    assert ref_points(coarse_case(True))[1].tolist() == [3, 3, 3, 3]


def test_launch_shape_cases_match_everything():
    for n1n, n2n in ((1, 1), (70, 70), (600, 600)):
        c = shape_case(n1n, n2n)
        c["ori"] = False
        n, m, codes = ref_points(c)
        assert n == n1n + 1 and set(codes.tolist()) == {ACCEPTED}
    c = shape_case(5, 5)
    assert ref_points(c, n1=0)[0] == 0
    n, m, codes = ref_points(c, n2=0)
    assert n == 0 and set(codes.tolist()) <= {NO_CANDIDATE}


def line_case(seed, n1=40, n2=40):
    rng = np.random.default_rng(seed)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    for q in range(0, min(n1, n2), 2):  # half the queries have a near copy
        d1[q] = flipped(d2[(q * 7) % n2], int(rng.integers(0, 40)), int(rng.integers(0, 200)))
    return d1, d2


def ref_lines(d1, d2, has1=None, has2=None, factor=0.1):
    n1, n2 = len(d1), len(d2)
    pairs = np.zeros((max(n1, 1), 2), np.int32)
    mad = np.zeros(2, np.float64)
    d1 = np.ascontiguousarray(d1, np.uint8)
    d2 = np.ascontiguousarray(d2, np.uint8)
    h1 = None if has1 is None else np.ascontiguousarray(has1, np.uint8)
    h2 = None if has2 is None else np.ascontiguousarray(has2, np.uint8)
    n = ref_lib().tri_ref_lines(_p(d1), n1, _p(d2), n2, None if h1 is None else _p(h1), None if h2 is None else _p(h2),
                                factor, _p(pairs), _p(mad))
    return pairs[:n].copy(), (float(mad[0]), float(mad[1]))


def knn_gap(d1, d2):
    """d1 - d0 of every query (numpy)."""
    dist = np.unpackbits(d1[:, None, :] ^ d2[None, :, :], axis=2).sum(2)
    s = np.sort(dist, axis=1)
    return s[:, 1] - s[:, 0], dist.argmin(1)


def line_masks(d1, d2, top=1):
    """Masks that hide the `top` queries with the largest d1 - d0, one more query, and two train lines in use."""
    gap, nn = knn_gap(d1, d2)
    h1 = np.zeros(len(d1), np.uint8)
    h2 = np.zeros(len(d2), np.uint8)
    h1[np.argsort(gap, kind="stable")[len(gap) - top:]] = 1
    h1[3] = 1
    h2[nn[0]] = 1
    h2[nn[6]] = 1
    return h1, h2


def test_line_restatement():
    d1, d2 = line_case(21)
    # with the init factor and no masks it is the oracle's SerachForInitialize
    pe, made = ol.line_search_init(d1, d2)
    pr, madr = ref_lines(d1, d2, factor=0.5)
    assert np.array_equal(pr, pe) and madr == made
    h1, h2 = line_masks(d1, d2)
    full, mad_full = ref_lines(d1, d2, np.zeros(40, np.uint8), np.zeros(40, np.uint8))
    masked, mad_masked = ref_lines(d1, d2, h1, h2)
    # the masks only remove pairs, after the MAD: it still counts the hidden queries
    assert mad_masked == mad_full and mad_full[1] > 0
    keep = [(q, t) for q, t in full.tolist() if not h1[q] and not h2[t]]
    assert masked.tolist() == [list(x) for x in keep] and 0 < len(masked) < len(full)
    qmax = int(knn_gap(d1, d2)[0].argmax())
    assert qmax in full[:, 0] and qmax not in masked[:, 0]
    # hiding the 15 largest gaps: the MAD is still the one over all 40 queries, not the one a matcher
    # would get by leaving the hidden queries out of the input
    h15 = line_masks(d1, d2, top=15)[0]
    assert ref_lines(d1, d2, h15, h2)[1] == mad_full and ref_lines(d1[h15 == 0], d2)[1][1] != mad_full[1]
    assert len(ref_lines(d1, d2[:1])[0]) == 0 and len(ref_lines(d1[:0], d2)[0]) == 0


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(GENERAL)), ids=["ori", "no-ori", "only-stereo"])
def test_gpu_general_parity(plvi_lib, i):
    c, (ne, me, _) = general(i)
    ng, mg = gpu_points(c)
    assert ng == ne and np.array_equal(mg, me)


@pytest.mark.gpu
def test_gpu_tie_rule_and_many_to_one(plvi_lib):
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0], []):
        check_gpu(tie_case(order))
    base = np.arange(32, dtype=np.uint8) * 5
    check_gpu(make_case([kp(10, 50), kp(30, 50)], [base, flipped(base, 2)], {4: [0, 1]}, [kp(300, 50), kp(310, 90)],
                        [base, flipped(base, 1)], {4: [0, 1]}))


@pytest.mark.gpu
def test_gpu_thresholds_and_flags(plvi_lib):
    inside, outside = np.nextafter(np.float32(10), np.float32(0)), np.nextafter(np.float32(10), np.float32(20))
    cases = [threshold_case(50), threshold_case(51), epipole_case(10.0), epipole_case(inside), epipole_case(outside),
             epipole_case(10.0, octave=1), epipole_case(inside, ur1=3.0), epipole_case(inside, ur2=0.0),
             stereo_flag_case(True), stereo_flag_case(False), coarse_case(False), coarse_case(True)]
    for c in cases:
        check_gpu(c)


@pytest.mark.gpu
def test_gpu_launch_shapes(plvi_lib):
    # nodes of 1, of more than a wave, and longer than the 512-thread staging / ownership stride (two slices)
    for n1n, n2n in ((1, 1), (70, 70), (600, 600), (3, 600), (600, 3)):
        check_gpu(shape_case(n1n, n2n))
    c = shape_case(5, 5)
    for key in ("kps1", "desc1", "has1", "ur1"):  # n1 = 0
        c[key] = c[key][:0]
    c["fv1"] = {}
    n, m = gpu_points(c)
    assert n == 0 and len(m) == 0
    c = shape_case(5, 5)
    for key in ("kps2", "desc2", "has2", "ur2"):  # n2 = 0
        c[key] = c[key][:0]
    c["fv2"] = {}
    n, m = gpu_points(c)
    assert n == 0 and np.array_equal(m, np.full(6, -1))


SENTINEL = 0x5A5A5A5A


def pack_side(cases, side, cap, node_cap, counts=None, node_counts=None):
    """Device tables of one side of a batch, in header order; padding rows hold junk."""
    P = len(cases)
    rng = np.random.default_rng(99)
    kps = np.frombuffer(rng.integers(0, 256, P * cap * 28, dtype=np.uint8).tobytes(), plvi.KEYPOINT_DTYPE).copy()
    kps = kps.reshape(P, cap)
    desc = rng.integers(0, 256, (P, cap, 32), dtype=np.uint8)
    has = rng.integers(0, 2, (P, cap), dtype=np.uint8)
    ur = rng.uniform(-5, 5, (P, cap)).astype(np.float32)
    node = rng.integers(0, 1000, (P, node_cap)).astype(np.int32)
    off = rng.integers(0, cap, (P, node_cap + 1)).astype(np.int32)
    idx = rng.integers(0, cap, (P, cap)).astype(np.int32)
    n = np.zeros(P, np.int32)
    nn = np.zeros(P, np.int32)
    for p, c in enumerate(cases):
        k = len(c["kps" + side])
        a, ao, ai = plvi.feature_vector_csr(c["fv" + side])
        kps[p, :k], desc[p, :k] = c["kps" + side], c["desc" + side]
        has[p, :k], ur[p, :k] = c["has" + side], c["ur" + side]
        node[p, :len(a)], off[p, :len(ao)], idx[p, :len(ai)] = a, ao, ai
        n[p], nn[p] = k, len(a)
    if counts is not None:
        n = np.asarray(counts, np.int32)
    if node_counts is not None:
        nn = np.asarray(node_counts, np.int32)
    arrays = [kps, desc, n, node, off, nn, idx, has, ur]
    bufs = [plvi.DeviceBuffer(a.nbytes) for a in arrays]
    for b, a in zip(bufs, arrays):
        b.upload(a)
    return bufs


@pytest.mark.gpu
def test_gpu_batch_of_six_unequal_pairs(plvi_lib):
    sizes = [(96, 80), (40, 96), (1, 33), (77, 1), (96, 96), (64, 50)]
    cases = [small_case(30 + i, a, b) for i, (a, b) in enumerate(sizes)]
    cap1 = cap2 = 96
    node_cap = max(max(len(c["fv1"]), len(c["fv2"])) for c in cases)
    assert node_cap == len(cases[4]["fv1"]) == len(cases[4]["fv2"])
    exp = [ref_points(c) for c in cases]
    assert sum(e[0] for e in exp) >= 20
    # pair 4 fills the tables: its counts are given above the capacities and must read as clamped
    n1 = [len(c["kps1"]) for c in cases]
    n2 = [len(c["kps2"]) for c in cases]
    nn1 = [len(c["fv1"]) for c in cases]
    nn2 = [len(c["fv2"]) for c in cases]
    n1[4], n2[4], nn1[4], nn2[4] = cap1 + 5, cap2 + 1000, node_cap + 3, node_cap + 1
    s1 = pack_side(cases, "1", cap1, node_cap, n1, nn1)
    s2 = pack_side(cases, "2", cap2, node_cap, n2, nn2)
    pairs = (plvi.TriangulationPair * 6)(*[pair_of(c) for c in cases])
    d_pairs = plvi.DeviceBuffer(ctypes.sizeof(pairs))
    d_pairs.upload(np.frombuffer(bytes(pairs), np.uint8))
    out = np.full((6, cap1), SENTINEL, np.int32)
    d_out, d_cnt = plvi.DeviceBuffer(out.nbytes), plvi.DeviceBuffer(24)
    d_out.upload(out)
    plvi.search_for_triangulation_batch(6, d_pairs.ptr, cap1, cap2, node_cap, [b.ptr for b in s1],
                                        [b.ptr for b in s2], d_out.ptr, d_cnt.ptr)
    plvi_lib.plvi_device_synchronize()
    got = d_out.download(np.zeros_like(out))
    cnt = d_cnt.download(np.zeros(6, np.int32))
    for p, (c, (ne, me, _)) in enumerate(zip(cases, exp)):
        k = len(c["kps1"])
        assert cnt[p] == ne and np.array_equal(got[p, :k], me), p
        assert (got[p, k:] == SENTINEL).all(), p  # rows past the count are never written
    # the LDS bound: 52 * cap2 + 16 * node_cap + 8 bytes against 160 KB, refused before any launch
    rc = plvi_lib.plvi_search_for_triangulation_batch(6, d_pairs.ptr, cap1, 4000, node_cap, *[b.ptr for b in s1],
                                                      *[b.ptr for b in s2], d_out.ptr, d_cnt.ptr, None)
    assert rc == plvi.PLVI_E_CAPACITY
    assert np.array_equal(d_out.download(np.zeros_like(out)), got)


@pytest.mark.gpu
def test_gpu_lines(plvi_lib):
    d1, d2 = line_case(21)
    h1, h2 = line_masks(d1, d2)
    h15 = line_masks(d1, d2, top=15)[0]
    for a, b in ((h1, h2), (np.zeros(40, np.uint8), np.zeros(40, np.uint8)), (h1, np.zeros(40, np.uint8)), (h15, h2)):
        pe, made = ref_lines(d1, d2, a, b)
        n, pg, madg = plvi.LineMatcher.SearchForTriangulation(d1, d2, a, b)
        assert n == len(pe) and np.array_equal(pg, pe) and madg == made
    for q, t in ((d1, d2[:1]), (d1[:0], d2), (d1, d2[:0])):  # n2 < 2, n1 = 0: 0 matches
        n, pg, _ = plvi.LineMatcher.SearchForTriangulation(q, t, np.zeros(len(q), np.uint8), np.zeros(len(t), np.uint8))
        assert n == 0 and len(pg) == 0


@pytest.mark.gpu
def test_gpu_lines_batch_of_four(plvi_lib):
    sets = [line_case(21), line_case(22, 33, 40), line_case(23, 40, 1), line_case(24, 0, 17)]
    cap1 = cap2 = 40
    rng = np.random.default_rng(7)
    D1 = rng.integers(0, 256, (4, cap1, 32), dtype=np.uint8)
    D2 = rng.integers(0, 256, (4, cap2, 32), dtype=np.uint8)
    H1 = rng.integers(0, 2, (4, cap1), dtype=np.uint8)
    H2 = rng.integers(0, 2, (4, cap2), dtype=np.uint8)
    exp = []
    for p, (a, b) in enumerate(sets):
        D1[p, :len(a)], D2[p, :len(b)] = a, b
        if p == 0:
            H1[0], H2[0] = line_masks(a, b)
        exp.append(ref_lines(a, b, H1[p, :len(a)], H2[p, :len(b)]))
    assert len(exp[0][0]) > 0 and len(exp[1][0]) > 0
    cnt = np.array([len(a) for a, _ in sets] + [len(b) for _, b in sets] + [0] * 4, np.int32)
    out = np.full((4, cap1, 2), SENTINEL, np.int32)
    arrays = [D1, D2, H1, H2, cnt, out]
    bufs = [plvi.DeviceBuffer(a.nbytes) for a in arrays]
    for bf, a in zip(bufs, arrays):
        bf.upload(a)
    scr, mad = plvi.DeviceBuffer(16 * 4 * cap1), plvi.DeviceBuffer(64)
    plvi.line_search_triangulation_batch(bufs[0].ptr, bufs[4].ptr, cap1, bufs[1].ptr, bufs[4].ptr + 16, cap2, 4,
                                         bufs[2].ptr, bufs[3].ptr, scr.ptr, bufs[5].ptr, bufs[4].ptr + 32, mad.ptr)
    plvi_lib.plvi_device_synchronize()
    got = bufs[5].download(np.zeros_like(out))
    ng = bufs[4].download(np.zeros(12, np.int32))[8:]
    madg = mad.download(np.zeros((4, 2), np.float64))
    for p, (pe, made) in enumerate(exp):
        assert ng[p] == len(pe) and np.array_equal(got[p, :len(pe)], pe) and tuple(madg[p]) == made, p
        assert (got[p, len(pe):] == SENTINEL).all(), p
