import math
import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def real_frames():
    z = np.load(GOLDEN / "frames.npz")
    return {k: z[k] for k in z.files}


def _assert_fields_same(kg, ke, tag):
    assert len(kg) == len(ke), f"{tag}: n {len(kg)} != {len(ke)}"
    for f in ke.dtype.names:
        a, b = kg[f], ke[f]
        bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32)) if a.dtype.kind == "f" else np.flatnonzero(a != b)
        assert bad.size == 0, f"{tag}: field {f} differs at {bad[:10]} got {a[bad[:5]]} exp {b[bad[:5]]}"


def assert_orb_same(got, exp, tag):
    """(monoIndex, keypoints, descriptors) of the HIP path vs the oracle's: monoIndex exactly, every
    cv::KeyPoint field bitwise in the reference's slot order, descriptors byte for byte."""
    mg, kg, dg = got
    me, ke, de = exp
    assert mg == me, f"{tag}: monoIndex {mg} != {me}"
    _assert_fields_same(kg, ke, tag)
    bad = np.flatnonzero((dg != de).any(axis=1))
    assert bad.size == 0, f"{tag}: descriptors differ at rows {bad[:10]}"


def assert_lines_same(got, exp, tag):
    """(keylines, descriptors, line functions) of the HIP path vs the oracle's: all 17 KeyLine fields
    bitwise, LBD descriptors byte for byte, the f64 line equations bitwise."""
    kg, dg, fg = got
    ke, de, fe = exp
    _assert_fields_same(kg, ke, tag)
    bad = np.flatnonzero((dg != de).any(axis=1))
    assert bad.size == 0, f"{tag}: descriptors differ at rows {bad[:10]}"
    bad = np.flatnonzero((fg.view(np.uint64) != fe.view(np.uint64)).any(axis=1))
    assert bad.size == 0, f"{tag}: line functions differ at rows {bad[:10]}"


def near_duplicate_descriptors(rng, n_train, n_query, frac=0.6, p_flip=0.08):
    """C3 generator: 60% of queries are train rows with
    Binomial(256, p) bit flips, the rest uniform random bits."""
    t = rng.integers(0, 256, size=(n_train, 32), dtype=np.uint8)
    q = rng.integers(0, 256, size=(n_query, 32), dtype=np.uint8)
    k = int(frac * n_query)
    src = rng.integers(0, n_train, size=k)
    bits = np.unpackbits(t[src], axis=1)
    flips = rng.random(bits.shape) < p_flip
    q[:k] = np.packbits(bits ^ flips, axis=1)
    return q, t


def bow_case(seed, n_kf=1000, n_f=1000, n_nodes=100, zipf=1.2, live=0.7, dup=0.6, flips=0.08, rot=20.0):
    """Synthetic SearchByBoW input: NodeIds from a Zipf
    over n_nodes, 70 % live MapPoints, dup of the F rows are KF rows with
    Binomial(256, flips) bit flips in the same node, angles rotated by `rot`
    degrees plus noise.  Returns (kf_desc, kf_angle, kf_live, kf_fv, f_desc,
    f_angle, f_fv) with fv = {node: [indices ascending]}."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n_nodes + 1) ** zipf
    w /= w.sum()
    node_ids = np.sort(rng.choice(100000, n_nodes, replace=False))
    kf_desc = rng.integers(0, 256, (n_kf, 32), dtype=np.uint8)
    kf_node = node_ids[rng.choice(n_nodes, n_kf, p=w)]
    kf_angle = rng.uniform(0, 360, n_kf).astype(np.float32)
    kf_live = (rng.random(n_kf) < live).astype(np.uint8)
    f_desc = rng.integers(0, 256, (n_f, 32), dtype=np.uint8)
    f_node = node_ids[rng.choice(n_nodes, n_f, p=w)]
    f_angle = rng.uniform(0, 360, n_f).astype(np.float32)
    nd = int(dup * n_f)
    src = rng.choice(n_kf, nd, replace=True)
    bits = np.unpackbits(kf_desc[src], axis=1)
    bits ^= (rng.random(bits.shape) < flips).astype(np.uint8)
    f_desc[:nd] = np.packbits(bits, axis=1)
    f_node[:nd] = kf_node[src]
    f_angle[:nd] = np.mod(kf_angle[src] - rot + rng.normal(0, 3, nd), 360).astype(np.float32)
    perm = rng.permutation(n_f)
    f_desc, f_node, f_angle = f_desc[perm], f_node[perm], f_angle[perm]

    def fv(nodes):
        d = {}
        for i, n in enumerate(nodes):
            d.setdefault(int(n), []).append(i)
        return d
    return kf_desc, kf_angle, kf_live, fv(kf_node), f_desc, f_angle, fv(f_node)


def line_iterator(x1, y1, x2, y2):
    """ORB_SLAM3::LineIterator (src/LineIterator.cpp:31-73): Bresenham on doubles."""
    steep = abs(y2 - y1) > abs(x2 - x1)
    if steep:
        x1, y1, x2, y2 = y1, x1, y2, x2
    if x1 > x2:
        x1, x2, y1, y2 = x2, x1, y2, y1
    dx, dy = x2 - x1, abs(y2 - y1)
    error = dx / 2.0
    ystep = 1 if y1 < y2 else -1
    x, y, maxX = int(x1), int(y1), int(x2)
    out = []
    while x <= maxX:
        out.append((y, x) if steep else (x, y))
        error -= dy
        if error < 0:
            y += ystep
            error += dx
        x += 1
    return out


def stereo_line_case(seed, n=220, W=640, H=480, cols=64, rows=48, ties=True):
    """Synthetic stereo line set shaped like Frame::ComputeStereoMatches_Lines
    (src/Frame.cc:1408-1451): right lines rasterised into the 64x48 grid with
    LineIterator, normalised directions, left lines = right lines shifted by a
    disparity with noisy descriptors.  Returns (lines1 int n1x4, desc1, grid,
    desc2, directions2)."""
    rng = np.random.default_rng(seed)
    inv_w, inv_h = cols / W, rows / H
    sp = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], 1)
    ang = rng.uniform(0, np.pi, n)
    ln = rng.uniform(5, 160, n)
    ep = np.clip(sp + np.stack([np.cos(ang), np.sin(ang)], 1) * ln[:, None], 0, [W - 1, H - 1])
    desc2 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if ties:  # duplicated right lines/descriptors produce distance ties
        k = n // 10
        desc2[-k:] = desc2[:k]
        sp[-k:] = sp[:k] + rng.normal(0, 2, (k, 2))
        ep[-k:] = ep[:k] + rng.normal(0, 2, (k, 2))
    grid = [[[] for _ in range(rows)] for _ in range(cols)]
    dirs = np.zeros((n, 2))
    for i in range(n):
        v = ((ep[i, 0] - sp[i, 0]) * inv_w, (ep[i, 1] - sp[i, 1]) * inv_h)
        m = np.sqrt(v[0] * v[0] + v[1] * v[1])
        dirs[i] = (v[0] / m, v[1] / m)
        for (x, y) in line_iterator(sp[i, 0] * inv_w, sp[i, 1] * inv_h, ep[i, 0] * inv_w, ep[i, 1] * inv_h):
            if 0 <= x < cols and 0 <= y < rows:
                grid[x][y].append(i)
    n1 = int(n * 0.9)
    src = rng.permutation(n)[:n1]
    disp = rng.uniform(2, 40, n1)
    s1 = sp[src] + np.stack([disp, np.zeros(n1)], 1)
    e1 = ep[src] + np.stack([disp, np.zeros(n1)], 1)
    bits = np.unpackbits(desc2[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.1).astype(np.uint8)
    desc1 = np.packbits(bits, axis=1)
    lines1 = np.stack([(s1[:, 0] * inv_w).astype(np.int64), (s1[:, 1] * inv_h).astype(np.int64),
                       (e1[:, 0] * inv_w).astype(np.int64), (e1[:, 1] * inv_h).astype(np.int64)], 1).astype(np.int32)
    return lines1, desc1, grid, desc2, dirs


def orb_scale_factors(n=8, sf=1.2):
    """ORBextractor mvScaleFactor (float cumulative, ORBextractor.cc:415-420)."""
    s = [np.float32(1.0)]
    for _ in range(1, n):
        s.append(np.float32(np.float64(s[-1]) * np.float64(np.float32(sf))))
    return np.array(s + [np.float32(0)] * (16 - n), np.float32)


def projection_case(seed, n_cur=1000, n_last=900, W=752, H=480, uright=False, dup=0.05):
    """Synthetic SearchByProjection input: current-frame
    keypoints (mvKeysUn) with descriptors; LastFrame MapPoints whose camera-
    frame positions project near a current keypoint (70 %) or anywhere (30 %),
    descriptors = the keypoint's with ~5 % bit flips (or random), a global
    rotation of 10 degrees; some points invalid / behind the camera / with
    Observations() == 0, some current keypoints pre-blocked, `dup` of the
    last points aimed at the same keypoint as another (assignment conflicts)."""
    from plvi import KEYPOINT_DTYPE, grid_geometry
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = np.float32(458.654), np.float32(457.296), np.float32(367.215), np.float32(248.375)
    kps = np.zeros(n_cur, KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(-4, W + 4, n_cur).astype(np.float32)
    kps["y"] = rng.uniform(-4, H + 4, n_cur).astype(np.float32)
    kps["octave"] = np.minimum(rng.geometric(0.35, n_cur) - 1, 7)
    kps["angle"] = rng.uniform(0, 360, n_cur).astype(np.float32)
    kps["size"] = 31
    kps["class_id"] = -1
    desc = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    near = rng.random(n_last) < 0.7
    src = rng.integers(0, n_cur, n_last)
    ndup = int(dup * n_last)
    src[:ndup] = src[ndup:2 * ndup]
    u = np.where(near, kps["x"][src] + rng.normal(0, 2.0, n_last), rng.uniform(0, W, n_last))
    v = np.where(near, kps["y"][src] + rng.normal(0, 2.0, n_last), rng.uniform(0, H, n_last))
    z = rng.uniform(1.0, 20.0, n_last)
    z[rng.random(n_last) < 0.02] *= -1
    x3 = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1).astype(np.float32)
    oct_ = np.clip(np.where(near, kps["octave"][src] + rng.integers(-1, 2, n_last), rng.integers(0, 8, n_last)), 0, 7)
    bits = np.unpackbits(desc[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.05).astype(np.uint8)
    mp = np.where(near[:, None], np.packbits(bits, axis=1), rng.integers(0, 256, (n_last, 32), dtype=np.uint8))
    ang = np.mod(kps["angle"][src] + 10 + rng.normal(0, 5, n_last), 360).astype(np.float32)
    flags = ((rng.random(n_last) < 0.92).astype(np.uint8) | ((rng.random(n_last) < 0.85).astype(np.uint8) << 1))
    case = {"cur_kps": kps, "cur_desc": desc, "cur_blocked": (rng.random(n_cur) < 0.05).astype(np.uint8),
            "cur_uright": None, "grid": grid_geometry(W, H), "scale_factors": orb_scale_factors(),
            "x3dc": x3, "flags": flags, "last_octave": oct_.astype(np.int32), "last_angle": ang,
            "mp_desc": mp.astype(np.uint8), "camera": (fx, fy, cx, cy, np.float32(40.0))}
    if uright:
        ur = np.where(rng.random(n_cur) < 0.6, kps["x"] - rng.uniform(0, 30, n_cur), -1).astype(np.float32)
        case["cur_uright"] = ur
    return case


KB8_TUMVI = (np.float32(190.978), np.float32(190.973), np.float32(254.932), np.float32(256.897),
             np.float32(0.0034823894), np.float32(0.00071503044), np.float32(-0.0020532361), np.float32(0.00020293143))


def _kb8_unproject(u, v, cam):
    """Rays (x/z, y/z) of pixels under KannalaBrandt8 (Newton on r(theta) = theta_d, float64)."""
    fx, fy, cx, cy, k1, k2, k3, k4 = (float(t) for t in cam)
    px, py = (u - cx) / fx, (v - cy) / fy
    td = np.minimum(np.hypot(px, py), np.pi / 2 - 1e-3)
    th = td.copy()
    for _ in range(20):
        t2 = th * th
        f = th * (1 + k1 * t2 + k2 * t2 ** 2 + k3 * t2 ** 3 + k4 * t2 ** 4) - td
        fd = 1 + 3 * k1 * t2 + 5 * k2 * t2 ** 2 + 7 * k3 * t2 ** 3 + 9 * k4 * t2 ** 4
        th = th - f / fd
    sc = np.where(td > 1e-8, np.tan(th) / np.maximum(td, 1e-12), 1.0)
    return px * sc, py * sc


def _kb8_project(x3, cam):
    fx, fy, cx, cy, k1, k2, k3, k4 = (float(t) for t in cam)
    x, y, z = x3[:, 0].astype(np.float64), x3[:, 1].astype(np.float64), x3[:, 2].astype(np.float64)
    th = np.arctan2(np.hypot(x, y), z)
    psi = np.arctan2(y, x)
    r = th + k1 * th ** 3 + k2 * th ** 5 + k3 * th ** 7 + k4 * th ** 9
    return fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy


def projection_stereo_case(seed, n_left=900, n_right=850, n_last=800, kb8=True, dup=0.05):
    """Two-camera SearchByProjection(CurrentFrame, LastFrame) input (CurrentFrame.Nleft != -1): a
    KannalaBrandt8 rig (TUM-VI-like intrinsics, 512 x 512, or a Pinhole one), left / right keypoints with
    descriptors, LastFrame points whose x3Dc project near a left keypoint (70 %) and whose x3Dr = Rrl x3Dc +
    trl project near a right keypoint placed there for 60 % of them (descriptor = the same source with flipped
    bits), a global 10-degree rotation, some points behind the camera / outliers / with Observations() == 0,
    pre-blocked keypoints on both sides, `dup` aimed at another point's keypoints."""
    from plvi import KEYPOINT_DTYPE
    rng = np.random.default_rng(seed)
    W = H = 512
    cam = KB8_TUMVI if kb8 else (np.float32(190.978), np.float32(190.973), np.float32(254.932),
                                 np.float32(256.897))

    def kset(n):
        k = np.zeros(n, KEYPOINT_DTYPE)
        k["x"] = rng.uniform(-4, W + 4, n).astype(np.float32)
        k["y"] = rng.uniform(-4, H + 4, n).astype(np.float32)
        k["octave"] = np.minimum(rng.geometric(0.35, n) - 1, 7)
        k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
        k["size"] = 31
        k["class_id"] = -1
        return k
    kl, kr = kset(n_left), kset(n_right)
    dl = rng.integers(0, 256, (n_left, 32), dtype=np.uint8)
    dr = rng.integers(0, 256, (n_right, 32), dtype=np.uint8)
    near = rng.random(n_last) < 0.7
    src = rng.integers(0, n_left, n_last)
    nd = int(dup * n_last)
    src[:nd] = src[nd:2 * nd]
    u = np.where(near, kl["x"][src] + rng.normal(0, 2.0, n_last), rng.uniform(0, W, n_last))
    v = np.where(near, kl["y"][src] + rng.normal(0, 2.0, n_last), rng.uniform(0, H, n_last))
    z = rng.uniform(1.0, 20.0, n_last)
    if kb8:
        rx_, ry_ = _kb8_unproject(u, v, cam)
    else:
        rx_, ry_ = (u - float(cam[2])) / float(cam[0]), (v - float(cam[3])) / float(cam[1])
    x3 = np.stack([rx_ * z, ry_ * z, z], 1)
    x3[rng.random(n_last) < 0.02] *= -1
    x3 = x3.astype(np.float32)
    a = np.deg2rad(2.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    x3r = (x3.astype(np.float64) @ R.T + np.array([-0.11, 0.002, 0.001])).astype(np.float32)
    if kb8:
        ur, vr = _kb8_project(x3r, cam)
    else:
        ur = float(cam[0]) * x3r[:, 0] / x3r[:, 2] + float(cam[2])
        vr = float(cam[1]) * x3r[:, 1] / x3r[:, 2] + float(cam[3])
    # right keypoints at the right projections of 60 % of the near points
    put = np.nonzero(near & (rng.random(n_last) < 0.6) & (x3[:, 2] > 0))[0][:n_right]
    slots = rng.choice(n_right, len(put), replace=False)
    kr["x"][slots] = (ur[put] + rng.normal(0, 1.5, len(put))).astype(np.float32)
    kr["y"][slots] = (vr[put] + rng.normal(0, 1.5, len(put))).astype(np.float32)
    kr["octave"][slots] = kl["octave"][src[put]]
    kr["angle"][slots] = np.mod(kl["angle"][src[put]] + rng.normal(0, 3, len(put)), 360).astype(np.float32)
    bits = np.unpackbits(dl[src[put]], axis=1)
    bits ^= (rng.random(bits.shape) < 0.04).astype(np.uint8)
    dr[slots] = np.packbits(bits, axis=1)
    oct_ = np.clip(np.where(near, kl["octave"][src] + rng.integers(-1, 2, n_last), rng.integers(0, 8, n_last)), 0, 7)
    bits = np.unpackbits(dl[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.05).astype(np.uint8)
    mp = np.where(near[:, None], np.packbits(bits, axis=1), rng.integers(0, 256, (n_last, 32), dtype=np.uint8))
    ang = np.mod(kl["angle"][src] + 10 + rng.normal(0, 5, n_last), 360).astype(np.float32)
    flags = ((rng.random(n_last) < 0.92).astype(np.uint8) | ((rng.random(n_last) < 0.85).astype(np.uint8) << 1))
    cols, rows = 64, 48
    grid = (np.float32(0), np.float32(W), np.float32(0), np.float32(H), np.float32(cols / W), np.float32(rows / H))
    return {"kps": kl, "desc": dl, "kps_r": kr, "desc_r": dr,
            "blocked": (rng.random(n_left) < 0.05).astype(np.uint8),
            "blocked_r": (rng.random(n_right) < 0.05).astype(np.uint8), "grid": grid,
            "scale_factors": orb_scale_factors(), "x3dc": x3, "x3dr": x3r, "flags": flags,
            "last_octave": oct_.astype(np.int32), "last_angle": ang, "mp_desc": mp.astype(np.uint8),
            "camera": tuple(cam[:4]) + (np.float32(0.0),), "kb8": np.array(cam[4:], np.float32) if kb8 else None}


def reloc_case(seed, n_cur=1000, n_kf=800, W=752, H=480, dup=0.08, pre_blocked=0.3):
    """Synthetic relocalization-search input (ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound,
    th, ORBdist), src/ORBmatcher.cc:2180-2300): current-frame keypoints (mvKeysUn) with descriptors, ~30 %
    already holding a MapPoint (the PnP inliers); KF MapPoints that project near a keypoint (70 %) or anywhere,
    descriptors = the keypoint's with ~6 % bit flips (or random), dist3D inside / outside the MapPoints'
    distance invariance range, PredictScale levels = the keypoint's octave +-1 (a few at the clamp ends), some
    points dead or already found, `dup` aimed at another point's keypoint (assignment conflicts), a global
    rotation of 10 degrees plus noise, points behind the camera (the reloc search has no depth test)."""
    from plvi import KEYPOINT_DTYPE, grid_geometry
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = np.float32(458.654), np.float32(457.296), np.float32(367.215), np.float32(248.375)
    kps = np.zeros(n_cur, KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(-4, W + 4, n_cur).astype(np.float32)
    kps["y"] = rng.uniform(-4, H + 4, n_cur).astype(np.float32)
    kps["octave"] = np.minimum(rng.geometric(0.35, n_cur) - 1, 7)
    kps["angle"] = rng.uniform(0, 360, n_cur).astype(np.float32)
    kps["size"] = 31
    kps["class_id"] = -1
    desc = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    near = rng.random(n_kf) < 0.7
    src = rng.integers(0, n_cur, n_kf)
    ndup = int(dup * n_kf)
    src[:ndup] = src[ndup:2 * ndup]
    u = np.where(near, kps["x"][src] + rng.normal(0, 2.0, n_kf), rng.uniform(-20, W + 20, n_kf))
    v = np.where(near, kps["y"][src] + rng.normal(0, 2.0, n_kf), rng.uniform(-20, H + 20, n_kf))
    z = rng.uniform(1.0, 20.0, n_kf)
    z[rng.random(n_kf) < 0.02] *= -1
    x3 = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1).astype(np.float32)
    d3 = np.abs(z * rng.uniform(1.0, 1.3, n_kf)).astype(np.float32)
    lo = (d3 * rng.uniform(0.3, 1.02, n_kf)).astype(np.float32)
    hi = (d3 * rng.uniform(0.98, 3.0, n_kf)).astype(np.float32)
    dist = np.stack([d3, lo, hi], 1).astype(np.float32)
    lvl = np.clip(np.where(near, kps["octave"][src] + rng.integers(-1, 2, n_kf), rng.integers(0, 8, n_kf)), 0, 7)
    bits = np.unpackbits(desc[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.06).astype(np.uint8)
    mp = np.where(near[:, None], np.packbits(bits, axis=1), rng.integers(0, 256, (n_kf, 32), dtype=np.uint8))
    ang = np.mod(kps["angle"][src] + 10 + rng.normal(0, 5, n_kf), 360).astype(np.float32)
    return {"cur_kps": kps, "cur_desc": desc, "cur_blocked": (rng.random(n_cur) < pre_blocked).astype(np.uint8),
            "grid": grid_geometry(W, H), "scale_factors": orb_scale_factors(), "x3dc": x3, "dist": dist,
            "level": lvl.astype(np.int32), "kf_flags": (rng.random(n_kf) < 0.9).astype(np.uint8),
            "kf_angle": ang, "mp_desc": mp.astype(np.uint8), "camera": (fx, fy, cx, cy, np.float32(0.0))}


def reloc_params(case, th, orb_dist):
    import plvi
    p = plvi.RelocParams()
    fx, fy, cx, cy, _ = case["camera"]
    p.fx, p.fy, p.cx, p.cy, p.th, p.orb_dist = fx, fy, cx, cy, th, orb_dist
    (p.min_x, p.max_x, p.min_y, p.max_y, p.inv_w, p.inv_h) = case["grid"]
    p.nlevels = len(case["scale_factors"])
    for i, s in enumerate(case["scale_factors"]):
        p.scale_factors[i] = s
    return p


def local_case(seed, n_cur=1000, n_mp=1500, W=752, H=480, uright=False, dup=0.15):
    """Synthetic local-map search input (ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>...),
    SURVEY 8f / VERDICT r1 item 8): current-frame keypoints with octaves and descriptors; MapPoints whose
    predicted projections fall near a keypoint (75 %) or anywhere, predicted level = the keypoint's octave
    +-1, descriptors = the keypoint's with ~6 % bit flips (ties and near-ties via duplicated MapPoints:
    `dup` of them aim at an earlier MapPoint's keypoint, so the sequential blocking matters), some not in
    view / bad, most with Observations() > 0, a few keypoints pre-blocked; view cosines on both sides of
    RadiusByViewingCos's 0.998."""
    from plvi import KEYPOINT_DTYPE, grid_geometry
    rng = np.random.default_rng(seed)
    kps = np.zeros(n_cur, KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(-3, W + 3, n_cur).astype(np.float32)
    kps["y"] = rng.uniform(-3, H + 3, n_cur).astype(np.float32)
    kps["octave"] = np.minimum(rng.geometric(0.35, n_cur) - 1, 7)
    kps["size"] = 31
    kps["class_id"] = -1
    desc = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    near = rng.random(n_mp) < 0.75
    src = rng.integers(0, n_cur, n_mp)
    nd = int(dup * n_mp)
    if nd:
        src[-nd:] = src[rng.integers(0, n_mp - nd, nd)]
    px = np.where(near, kps["x"][src] + rng.normal(0, 1.5, n_mp), rng.uniform(0, W, n_mp)).astype(np.float32)
    py = np.where(near, kps["y"][src] + rng.normal(0, 1.5, n_mp), rng.uniform(0, H, n_mp)).astype(np.float32)
    pxr = (px - rng.uniform(0, 30, n_mp)).astype(np.float32)
    vc = np.where(rng.random(n_mp) < 0.5, rng.uniform(0.999, 1.0, n_mp), rng.uniform(0.5, 0.998, n_mp)).astype(
        np.float32)
    lvl = np.clip(np.where(near, kps["octave"][src] + rng.integers(-1, 2, n_mp), rng.integers(0, 8, n_mp)), 0, 7)
    bits = np.unpackbits(desc[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.06).astype(np.uint8)
    md = np.where(near[:, None], np.packbits(bits, axis=1), rng.integers(0, 256, (n_mp, 32), dtype=np.uint8))
    flags = ((rng.random(n_mp) < 0.9).astype(np.uint8) | ((rng.random(n_mp) < 0.85).astype(np.uint8) << 1))
    case = {"cur_kps": kps, "cur_desc": desc, "cur_blocked": (rng.random(n_cur) < 0.05).astype(np.uint8),
            "cur_uright": None, "grid": grid_geometry(W, H), "scale_factors": orb_scale_factors(),
            "mp_flags": flags, "mp_proj": np.stack([px, py, pxr, vc], 1).astype(np.float32),
            "mp_level": lvl.astype(np.int32), "mp_desc": md.astype(np.uint8)}
    if uright:
        case["cur_uright"] = np.where(rng.random(n_cur) < 0.6, kps["x"] - rng.uniform(0, 30, n_cur), -1).astype(
            np.float32)
    return case


def local_stereo_case(seed, n_left=900, n_right=850, n_mp=1400, W=752, H=480, pair_frac=0.6, dup=0.15):
    """Two-camera local-map search input (F.Nleft != -1): left / right keypoint sets with descriptors, a
    fraction of them paired (mvLeftToRightMatch / mvRightToLeftMatch, mutually consistent, right
    descriptor = the left one with a few flipped bits); MapPoints seen in the left image, the right image or
    both (bit0 / bit2), each aiming near a keypoint of that image (its predicted level = the keypoint's
    octave +-1, the right level sometimes -1), duplicates aiming at an earlier MapPoint's keypoints so the
    sequential blocking and the stereo cross-assignments matter."""
    from plvi import KEYPOINT_DTYPE, grid_geometry
    rng = np.random.default_rng(seed)

    def kset(n):
        k = np.zeros(n, KEYPOINT_DTYPE)
        k["x"] = rng.uniform(-3, W + 3, n).astype(np.float32)
        k["y"] = rng.uniform(-3, H + 3, n).astype(np.float32)
        k["octave"] = np.minimum(rng.geometric(0.35, n) - 1, 7)
        k["size"] = 31
        k["class_id"] = -1
        return k
    kl, kr = kset(n_left), kset(n_right)
    dl = rng.integers(0, 256, (n_left, 32), dtype=np.uint8)
    dr = rng.integers(0, 256, (n_right, 32), dtype=np.uint8)
    npair = int(pair_frac * min(n_left, n_right))
    li = rng.choice(n_left, npair, replace=False)
    ri = rng.choice(n_right, npair, replace=False)
    l2r = np.full(n_left, -1, np.int32)
    r2l = np.full(n_right, -1, np.int32)
    l2r[li] = ri
    r2l[ri] = li
    bits = np.unpackbits(dl[li], axis=1)
    bits ^= (rng.random(bits.shape) < 0.03).astype(np.uint8)
    dr[ri] = np.packbits(bits, axis=1)
    kr["octave"][ri] = kl["octave"][li]

    def aim(k, d, n):
        near = rng.random(n_mp) < 0.8
        src = rng.integers(0, n, n_mp)
        nd = int(dup * n_mp)
        if nd:
            src[-nd:] = src[rng.integers(0, n_mp - nd, nd)]
        px = np.where(near, k["x"][src] + rng.normal(0, 1.5, n_mp), rng.uniform(0, W, n_mp)).astype(np.float32)
        py = np.where(near, k["y"][src] + rng.normal(0, 1.5, n_mp), rng.uniform(0, H, n_mp)).astype(np.float32)
        vc = np.where(rng.random(n_mp) < 0.5, rng.uniform(0.999, 1.0, n_mp), rng.uniform(0.5, 0.998, n_mp))
        lvl = np.clip(np.where(near, k["octave"][src] + rng.integers(-1, 2, n_mp), rng.integers(0, 8, n_mp)), 0, 7)
        return src, near, np.stack([px, py, np.zeros(n_mp), vc], 1).astype(np.float32), lvl.astype(np.int32)
    srcl, nearl, prl, lvl = aim(kl, dl, n_left)
    srcr, nearr, prr, lvr = aim(kr, dr, n_right)
    side = rng.random(n_mp)  # left only / right only / both
    bl = side < 0.75
    br = side > 0.45
    # a MapPoint seen in both images aims at a stereo pair's two keypoints when its left target has one
    both = bl & br & (l2r[srcl] >= 0)
    srcr = np.where(both, l2r[srcl], srcr)
    prr[both, 0] = kr["x"][srcr[both]] + rng.normal(0, 1.5, both.sum()).astype(np.float32)
    prr[both, 1] = kr["y"][srcr[both]] + rng.normal(0, 1.5, both.sum()).astype(np.float32)
    nearr = nearr | both
    lvr = np.where(both, np.clip(kr["octave"][srcr] + rng.integers(-1, 2, n_mp), 0, 7), lvr).astype(np.int32)
    lvr = np.where(rng.random(n_mp) < 0.05, -1, lvr).astype(np.int32)
    base = np.where(bl, dl[srcl].T, dr[srcr].T).T
    bits = np.unpackbits(base, axis=1)
    bits ^= (rng.random(bits.shape) < 0.06).astype(np.uint8)
    md = np.where((nearl | nearr)[:, None], np.packbits(bits, axis=1),
                  rng.integers(0, 256, (n_mp, 32), dtype=np.uint8))
    alive = rng.random(n_mp) < 0.92
    obs = rng.random(n_mp) < 0.85
    flags = ((bl & alive).astype(np.uint8) | (obs.astype(np.uint8) << 1) | ((br & alive).astype(np.uint8) << 2))
    return {"kps": kl, "desc": dl, "kps_r": kr, "desc_r": dr, "l2r": l2r, "r2l": r2l,
            "blocked": (rng.random(n_left) < 0.04).astype(np.uint8),
            "blocked_r": (rng.random(n_right) < 0.04).astype(np.uint8),
            "grid": grid_geometry(W, H), "scale_factors": orb_scale_factors(),
            "mp_flags": flags, "mp_proj": prl, "mp_level": lvl, "mp_proj_r": prr, "mp_level_r": lvr,
            "mp_desc": md.astype(np.uint8)}


def local_params(case, th):
    import plvi
    p = plvi.LocalParams()
    min_x, _, min_y, _, inv_w, inv_h = case["grid"]
    p.min_x, p.min_y, p.inv_w, p.inv_h, p.th, p.nlevels = min_x, min_y, inv_w, inv_h, th, 8
    for i, s in enumerate(case["scale_factors"]):
        p.scale_factors[i] = s
    return p


def line_proj_case(seed, n_cur=200, n_last=180, W=640, H=480, cols=64, rows=48):
    """Synthetic LineMatcher::SearchByProjection input: current-frame lines rasterised into the 64 x 48
    grid_Line with LineIterator (angles = atan2f of their endpoints, as KeyLine.angle), last-frame MapLines
    whose camera-frame endpoints project near a current line's (80 %) or anywhere, descriptors = the
    line's with ~8 % bit flips, duplicates aiming at the same current line (blocking order), some outliers
    / behind the camera / Observations() == 0, a few current lines pre-blocked."""
    rng = np.random.default_rng(seed)
    inv_w, inv_h = cols / W, rows / H
    sp = np.stack([rng.uniform(0, W - 1, n_cur), rng.uniform(0, H - 1, n_cur)], 1)
    ang = rng.uniform(0, 2 * np.pi, n_cur)
    ln = rng.uniform(10, 150, n_cur)
    ep = np.clip(sp + np.stack([np.cos(ang), np.sin(ang)], 1) * ln[:, None], 0, [W - 1, H - 1])
    sp32, ep32 = sp.astype(np.float32), ep.astype(np.float32)
    cur_angle = np.arctan2(ep32[:, 1] - sp32[:, 1], ep32[:, 0] - sp32[:, 0]).astype(np.float32)
    grid = [[[] for _ in range(rows)] for _ in range(cols)]
    for i in range(n_cur):
        for (x, y) in line_iterator(sp[i, 0] * inv_w, sp[i, 1] * inv_h, ep[i, 0] * inv_w, ep[i, 1] * inv_h):
            if 0 <= x < cols and 0 <= y < rows:
                grid[x][y].append(i)
    cur_desc = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    fx, fy, cx, cy = np.float32(458.654), np.float32(457.296), np.float32(320.0), np.float32(240.0)
    near = rng.random(n_last) < 0.8
    src = rng.integers(0, n_cur, n_last)
    k = n_last // 8
    src[-k:] = src[:k]
    x3 = np.zeros((n_last, 6), np.float32)
    for i in range(n_last):
        for e, P in enumerate((sp, ep)):
            u, v = (P[src[i]] + rng.normal(0, 1.0, 2)) if near[i] else rng.uniform([0, 0], [W, H])
            z = rng.uniform(1.0, 15.0)
            x3[i, 3 * e:3 * e + 3] = ((u - cx) * z / fx, (v - cy) * z / fy, z)
    x3[rng.random(n_last) < 0.03, 2] *= -1
    bits = np.unpackbits(cur_desc[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.08).astype(np.uint8)
    ml = np.where(near[:, None], np.packbits(bits, axis=1), rng.integers(0, 256, (n_last, 32), dtype=np.uint8))
    flags = ((rng.random(n_last) < 0.92).astype(np.uint8) | ((rng.random(n_last) < 0.85).astype(np.uint8) << 1))
    return {"cur_angle": cur_angle, "cur_desc": cur_desc, "cur_blocked": (rng.random(n_cur) < 0.05).astype(np.uint8),
            "grid": grid, "last_flags": flags, "x3dc": x3,
            "last_octave": (rng.random(n_last) < 0.3).astype(np.int32), "ml_desc": ml.astype(np.uint8),
            "scale_l": np.array([1, 2, 0, 0, 0, 0, 0, 0], np.float32), "camera": (fx, fy, cx, cy),
            "bounds": (np.float32(0), np.float32(W), np.float32(0), np.float32(H)), "inv_w": inv_w, "inv_h": inv_h}


def line_proj_params(case, th, angth, range_hint=1):
    import plvi
    p = plvi.LineProjParams()
    p.fx, p.fy, p.cx, p.cy = case["camera"]
    p.min_x, p.max_x, p.min_y, p.max_y = case["bounds"]
    p.inv_w, p.inv_h, p.th, p.angth, p.range_hint, p.nlevels = case["inv_w"], case["inv_h"], th, angth, range_hint, 2
    for i, s in enumerate(case["scale_l"]):
        p.scale_l[i] = s
    return p


def proj_params(case, th, forward=0, backward=0):
    import plvi
    p = plvi.ProjParams()
    fx, fy, cx, cy, mbf = case["camera"]
    p.fx, p.fy, p.cx, p.cy, p.mbf, p.th = fx, fy, cx, cy, mbf, th
    (p.min_x, p.max_x, p.min_y, p.max_y, p.inv_w, p.inv_h) = case["grid"]
    p.forward, p.backward, p.nlevels = forward, backward, 8
    for i, s in enumerate(case["scale_factors"]):
        p.scale_factors[i] = s
    return p


def structured_frames(w=640, h=480):
    """Extreme-contrast 640x480 cases: a 0/255 vertical step, a 0/255
    checkerboard of 40-pixel squares, 3-pixel diagonal stripes and binary
    (0/255) noise -- gradients at the u8 maximum, lines running into the
    image border, and FAST / region-growing thresholds met almost everywhere."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {}
    out["step"] = np.where(xx < w // 2 + 3, 0, 255).astype(np.uint8)
    out["checker"] = np.where(((xx // 40) + (yy // 40)) % 2 == 0, 0, 255).astype(np.uint8)
    out["stripes"] = np.where(((xx + yy) // 3) % 2 == 0, 30, 220).astype(np.uint8)
    rng = np.random.default_rng(11)
    out["binary_noise"] = (rng.integers(0, 2, size=(h, w)) * 255).astype(np.uint8)
    return out


# Exact fused multiply-add (Python 3.10 has no math.fma): the reference build
# fuses some `a*b + c` sites (oracle/ref_fma.h, tests/test_ref_objects.py);
# the pure-Python restatements use these at the same sites.
def fma(a, b, c):
    """a*b + c rounded once to double (float(Fraction) is correctly rounded)."""
    from fractions import Fraction
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))  # inf / NaN: as the unfused operations
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fmaf(a, b, c):
    """a*b + c on float32 operands rounded once to float32 (ties to even)."""
    from fractions import Fraction
    exact = Fraction(float(np.float32(a))) * Fraction(float(np.float32(b))) + Fraction(float(np.float32(c)))
    f = np.float32(float(exact))  # double then float32: may double-round, fixed below
    best = f
    for g in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        dg, db = abs(Fraction(float(g)) - exact), abs(Fraction(float(best)) - exact)
        if dg < db or (dg == db and (int(np.float32(g).view(np.uint32)) & 1) == 0):
            best = g
    return np.float32(best)


# ------------------------------------------------------------- frustum cases
def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def frustum_params(seed, model=0, two_camera=False, far_points=False, compat=0, nlevels=8, scale=1.2):
    """plvi_frustum_params of a synthetic frame: random pose (Rcw, tcw, Ow = -Rcw^T tcw as float), EuRoC-like
    Pinhole (752 x 480, mbf = 0.11 fx) or TUM-VI-like KannalaBrandt8 (512 x 512); two_camera adds a right
    camera 0.1 m to the side (R = Rrl Rcw, t = Rrl tcw + trl, O = Rwc tlr + Ow) with a slight rotation."""
    import plvi
    rng = np.random.default_rng(seed)
    p = plvi.FrustumParams()
    R = _rotation(rng)
    t = rng.normal(0, 2, 3)
    Ow = -R.T @ t

    def set_cam(c, R_, t_, O_):
        for i in range(9):
            c.R[i] = np.float32(R_.flat[i])
        for i in range(3):
            c.t[i] = np.float32(t_[i])
            c.O[i] = np.float32(O_[i])
        if model == 0:
            c.fx, c.fy, c.cx, c.cy = 458.654, 457.296, 367.215, 248.375
        else:
            c.fx, c.fy, c.cx, c.cy = (float(v) for v in KB8_TUMVI[:4])
            for i in range(4):
                c.kb[i] = KB8_TUMVI[4 + i]
        c.model = model

    set_cam(p.cam[0], R, t, Ow)
    if two_camera:
        a = 0.02
        Rrl = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        trl = np.array([-0.101, 0.002, 0.001])
        tlr = -Rrl.T @ trl
        set_cam(p.cam[1], Rrl @ R, Rrl @ t + trl, R.T @ tlr + Ow)
    p.two_camera = int(two_camera)
    p.mbf = np.float32(0.11) * np.float32(p.cam[0].fx) if model == 0 else 0.0
    if model == 0:
        p.min_x, p.max_x, p.min_y, p.max_y = -0.75, 752.5, 0.25, 479.25
    else:
        p.min_x, p.max_x, p.min_y, p.max_y = 0.0, 512.0, 0.0, 512.0
    p.view_cos_limit = 0.5
    p.far_points, p.far_th = int(far_points), 9.0
    p.nlevels = nlevels
    p.log_scale_factor = float(np.float32(np.log(np.float32(scale))))
    p.compat = compat
    plvi.frustum_params_init(p)
    return p


def _cam_points(rng, n, model):
    """Camera-frame points: most in front and inside / around the field of view, some behind."""
    z = np.where(rng.random(n) < 0.1, rng.uniform(-3, 0, n), rng.uniform(0.05, 25, n))
    s = 0.9 if model == 0 else 2.5
    return np.stack([z * rng.uniform(-s, s, n), z * rng.uniform(-s * 0.7, s * 0.7, n), z], 1)


def _world(p, pc, cam=0):
    c = p.cam[cam]
    R = np.array(c.R[:], np.float64).reshape(3, 3)
    t = np.array(c.t[:], np.float64)
    return (pc - t) @ R  # R^T (pc - t)


def _normals(rng, po):
    """Unit normals at ~0-90 degrees from the viewing ray PO (the view cos straddles 0.5)."""
    u = po / np.maximum(np.linalg.norm(po, axis=1, keepdims=True), 1e-12)
    perp = np.cross(u, rng.normal(size=u.shape))
    perp /= np.maximum(np.linalg.norm(perp, axis=1, keepdims=True), 1e-12)
    a = rng.uniform(0, np.pi / 2, len(u))
    return (u * np.cos(a)[:, None] + perp * np.sin(a)[:, None]).astype(np.float32)


def frustum_case(seed, p, n=3000):
    """Local MapPoints of frame p (Tracking::SearchLocalPoints input): world positions, normals, {mfMinDistance,
    mfMaxDistance} straddling the 0.8 / 1.2 invariance bounds with max/dist ratios over every level, flags,
    and stale MapPoint fields from an earlier frame; plus degenerate points (camera centre, zero depth)."""
    rng = np.random.default_rng(seed)
    model = p.cam[0].model
    pw = _world(p, _cam_points(rng, n, model)).astype(np.float32)
    O = np.array(p.cam[0].O[:], np.float32)
    d = np.linalg.norm(pw.astype(np.float64) - O, axis=1)
    mx = d * 1.2 ** rng.uniform(-1.3, 8.5, n)
    mn = d / 0.8 * 1.2 ** rng.uniform(-8, 0.4, n)
    # degenerate: the camera centre itself (Pc ~ 0, dist 0), zero max / min distance
    pw[:4] = O
    mx[:2], mn[:4] = 0.0, 0.0
    dist = np.stack([mn, mx], 1).astype(np.float32)
    case = {"pos": pw, "normal": _normals(rng, pw.astype(np.float64) - O), "dist": dist,
            "in_flags": ((rng.random(n) < 0.9).astype(np.uint8) | ((rng.random(n) < 0.85).astype(np.uint8) << 1)),
            "proj": rng.uniform(-5, 800, (n, 4)).astype(np.float32), "level": rng.integers(-1, 8, n).astype(np.int32),
            "depth": rng.uniform(0, 30, n).astype(np.float32),
            "proj_r": rng.uniform(-5, 800, (n, 4)).astype(np.float32),
            "level_r": rng.integers(-1, 8, n).astype(np.int32)}
    case["in_flags"][:4] |= 1
    return case


def frustum_line_case(seed, p, n=800):
    """Local MapLines of frame p: world endpoints (double) of segments in front / behind / across the image
    border, float normals, {mfMinDistance, mfMaxDistance}, evaluated flags, descriptors, stale fields."""
    rng = np.random.default_rng(seed)
    a = _cam_points(rng, n, 0)
    b = a + rng.normal(0, 1.0, (n, 3)) * np.maximum(a[:, 2:3], 0.5) * 0.3
    sp, ep = _world(p, a), _world(p, b)
    O = np.array(p.cam[0].O[:], np.float64)
    mid = (sp + ep) / 2 - O
    d = np.linalg.norm(mid, axis=1)
    dist = np.stack([d / 0.8 * 1.2 ** rng.uniform(-6, 0.4, n), d * 1.2 ** rng.uniform(-1.3, 6, n)], 1)
    return {"sep": np.concatenate([sp, ep], 1), "normal": _normals(rng, mid), "dist": dist.astype(np.float32),
            "in_flags": (rng.random(n) < 0.9).astype(np.uint8),
            "desc": rng.integers(0, 256, (n, 32), dtype=np.uint8),
            "proj": rng.uniform(-5, 800, (n, 4)).astype(np.float32), "angle": rng.uniform(-3, 3, n)}


# ------------------------------------------------------------- rectified stereo
# Literal pure-Python restatements of Frame::ComputeStereoMatches (src/Frame.cc:1228-1406) and
# Frame::ComputeStereoMatches_Lines (:1408-1492, lineSegmentOverlapStereo :1494-1529,
# filterLineSegmentDisparity :1531-1542).  tests/test_stereo.py pins the oracle against them on extractor
# output; tests/test_stereo_branches.py on crafted pairs, where the traced variants also say which branch
# every left keypoint / line took.
_f32 = np.float32

# outcome of a left keypoint (py_stereo_traced)
(ST_NO_CANDIDATE, ST_MAXU_NEG, ST_NO_ORB_MATCH, ST_BORDER_SKIP, ST_EDGE_MINIMUM, ST_DELTA_RANGE, ST_DISPARITY_RANGE,
 ST_CLAMPED, ST_ACCEPTED, ST_MEDIAN_REJECTED) = range(10)
ST_NAMES = ("NO_CANDIDATE", "MAXU_NEG", "NO_ORB_MATCH", "BORDER_SKIP", "EDGE_MINIMUM", "DELTA_RANGE",
            "DISPARITY_RANGE", "CLAMPED", "ACCEPTED", "MEDIAN_REJECTED")

# outcome of a left line (py_stereo_lines_traced): the first test of the acceptance condition that fails, the
# two horizontal tests first; and the arm of lineSegmentOverlapStereo it took
(SL_UNMATCHED, SL_HORIZONTAL_LEFT, SL_HORIZONTAL_RIGHT, SL_RATIO_REJECT, SL_MIN_DISP_REJECT, SL_OVERLAP_REJECT,
 SL_ACCEPTED) = range(7)
SL_NAMES = ("UNMATCHED", "HORIZONTAL_LEFT", "HORIZONTAL_RIGHT", "RATIO_REJECT", "MIN_DISP_REJECT", "OVERLAP_REJECT",
            "ACCEPTED")
OV_NONE, OV_DISJOINT, OV_CONTAINED, OV_PARTIAL, OV_SHORT_LENGTH = range(5)
OV_NAMES = ("NONE", "DISJOINT", "CONTAINED", "PARTIAL", "SHORT_LENGTH")

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def py_stereo_traced(kL, dL, kR, dR, pyrL, pyrR, scale, inv, mb, mbf):
    """Literal restatement of Frame::ComputeStereoMatches (float32 arithmetic).  Returns (mvuRight, mvDepth,
    codes, info): codes[iL] = the ST_* outcome of left keypoint iL (ST_CLAMPED / ST_ACCEPTED are kept matches,
    ST_MEDIAN_REJECTED a match the median test removed); info = {"sad": the accepted SADs in iL order,
    "sad_idx": their iL, "clamped": mask of the matches that took the disparity <= 0 clamp, "best": the chosen
    right index per left keypoint (-1 none), "band": (minr, maxr) per right keypoint, "pre": the outcomes before
    the median test}."""
    N = len(kL)
    ur = np.full(N, -1, np.float32)
    dp = np.full(N, -1, np.float32)
    codes = np.full(N, ST_NO_CANDIDATE, np.int32)
    clamped = np.zeros(N, bool)
    bestidx = np.full(N, -1, np.int32)
    nRows = pyrL[0].shape[0]
    rows = [[] for _ in range(nRows)]
    band = np.zeros((len(kR), 2), np.int64)
    for iR in range(len(kR)):
        y = _f32(kR["y"][iR])
        sc = _f32(scale[kR["octave"][iR]])  # kpY +/- 2*scale, fused in Frame.cc.o
        maxr, minr = int(math.ceil(fmaf(2.0, sc, y))), int(math.floor(fmaf(-2.0, sc, y)))
        band[iR] = (minr, maxr)
        for yi in range(minr, maxr + 1):
            rows[yi].append(iR)
    minD, maxD = _f32(0), _f32(mbf / mb)
    vdist = []
    dL = np.asarray(dL, np.uint8).reshape(-1, 32)
    dR = np.asarray(dR, np.uint8).reshape(-1, 32)
    for iL in range(N):
        lev, vL, uL = int(kL["octave"][iL]), _f32(kL["y"][iL]), _f32(kL["x"][iL])
        cand = rows[int(vL)]
        if not cand:
            continue
        minU, maxU = _f32(uL - maxD), _f32(uL - minD)
        if maxU < 0:
            codes[iL] = ST_MAXU_NEG
            continue
        best, bestR = 100, 0
        dists_c = _POP8[dR[cand] ^ dL[iL]].sum(1)  # DescriptorDistance to every candidate
        for c, iR in enumerate(cand):
            if kR["octave"][iR] < lev - 1 or kR["octave"][iR] > lev + 1:
                continue
            uR = _f32(kR["x"][iR])
            if minU <= uR <= maxU:
                d = int(dists_c[c])
                if d < best:
                    best, bestR = d, iR
        if best >= 75:
            codes[iL] = ST_NO_ORB_MATCH
            continue
        bestidx[iL] = bestR
        sf = inv[lev]
        rnd = lambda v: _f32(math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5))  # noqa: E731
        suL, svL, suR0 = rnd(_f32(uL * sf)), rnd(_f32(vL * sf)), rnd(_f32(_f32(kR["x"][bestR]) * sf))
        w, L = 5, 5
        IL = pyrL[lev][int(svL) - w:int(svL) + w + 1, int(suL) - w:int(suL) + w + 1].astype(np.int32)
        IL = IL - IL[w, w]
        if suR0 < 0 or suR0 + L + w + 1 >= pyrR[lev].shape[1]:
            codes[iL] = ST_BORDER_SKIP
            continue
        dists = []
        for inc in range(-L, L + 1):
            c = int(suR0 + inc - w)
            IR = pyrR[lev][int(svL) - w:int(svL) + w + 1, c:c + 2 * w + 1].astype(np.int32)
            IR = IR - IR[w, w]
            dists.append(_f32(np.abs(IL - IR).sum()))
        bi = int(np.argmin(dists))  # first minimum = strict-< scan
        binc = bi - L
        if binc in (-L, L):
            codes[iL] = ST_EDGE_MINIMUM
            continue
        d1, d2, d3 = dists[bi - 1], dists[bi], dists[bi + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = _f32(_f32(d1 - d3) / _f32(_f32(2.0) * fmaf(-2.0, d2, _f32(d1 + d3))))
        if delta < -1 or delta > 1:
            codes[iL] = ST_DELTA_RANGE
            continue
        bu = _f32(scale[lev] * _f32(_f32(suR0 + _f32(binc)) + delta))
        disp = _f32(uL - bu)
        if disp >= minD and disp < maxD:
            codes[iL] = ST_ACCEPTED
            if disp <= 0:
                disp, bu = _f32(0.01), _f32(float(uL) - 0.01)
                codes[iL] = ST_CLAMPED
                clamped[iL] = True
            dp[iL], ur[iL] = _f32(mbf / disp), bu
            vdist.append((int(d2), iL))
        else:
            codes[iL] = ST_DISPARITY_RANGE
    info = {"sad": np.array([d for d, _ in vdist], np.int64), "sad_idx": np.array([i for _, i in vdist], np.int64),
            "clamped": clamped, "best": bestidx, "band": band, "pre": codes.copy()}
    if vdist:
        vdist.sort()
        th = _f32(_f32(_f32(1.5) * _f32(1.4)) * _f32(vdist[len(vdist) // 2][0]))
        for d, i in reversed(vdist):
            if _f32(d) < th:
                break
            ur[i] = dp[i] = -1
            codes[i] = ST_MEDIAN_REJECTED
    return ur, dp, codes, info


def py_stereo(kL, dL, kR, dR, pyrL, pyrR, scale, inv, mb, mbf):
    """(mvuRight, mvDepth) of py_stereo_traced."""
    return py_stereo_traced(kL, dL, kR, dR, pyrL, pyrR, scale, inv, mb, mbf)[:2]


def py_overlap_traced(spl, epl, spp, epp):
    """Frame::lineSegmentOverlapStereo -> (overlap, OV_* arm)."""
    ov, arm = 1.0, OV_NONE
    if abs(epl - spl) > float(_f32(0.1)):
        sln, eln, spn, epn = min(spl, epl), max(spl, epl), min(spp, epp), max(spp, epp)
        length = eln - spn
        if epn < sln or spn > eln:
            ov, arm = 0.0, OV_DISJOINT
        elif epn > eln and spn < sln:
            ov, arm = eln - sln, OV_CONTAINED
        else:
            ov, arm = min(eln, epn) - max(sln, spn), OV_PARTIAL
        if length > float(_f32(0.01)):
            ov = ov / length
        else:
            ov, arm = 0.0, OV_SHORT_LENGTH
        ov = min(ov, 1.0) if ov > 1.0 else ov
    return ov, arm


def py_overlap(spl, epl, spp, epp):
    return py_overlap_traced(spl, epl, spp, epp)[0]


def py_stereo_lines_traced(klL, dL, klR, dR, W, H, mbf, klUn=None, range_hint=0):
    """Restatement of ComputeStereoMatches_Lines around oracle_lib.match_grid.  Returns (matches_12,
    mvDisparity_l, mvDepth_l, codes, info): codes[i1] = SL_* outcome; info = {"arm": OV_* per left line, "le":
    mvle_l from klUn (None = the left lines), "grid_total": entries of the right lines' GridStructure,
    "cells_outside": rasterised cells that fell outside it, "max_cell": the longest cell list, "quirk": mask of
    the lines whose acceptance differs when ep_r is re-projected from the original sp_r instead of the
    updated one (Frame.cc:1469-1470), "disp": the (disp_s, disp_e) doubles before the filter}."""
    import oracle_lib
    iw, ih = 64 / W, 48 / H
    n1, n2 = len(klL), len(klR)
    g = lambda k, f: k[f].astype(np.float64)  # noqa: E731
    sx, sy, ex, ey = g(klL, "startPointX"), g(klL, "startPointY"), g(klL, "endPointX"), g(klL, "endPointY")
    with np.errstate(invalid="ignore"):
        lines1 = np.stack([np.trunc(sx * iw), np.trunc(sy * ih), np.trunc(ex * iw), np.trunc(ey * ih)],
                          1).astype(np.int64).astype(np.int32)
    grid = [[[] for _ in range(48)] for _ in range(64)]
    dirs = np.zeros((n2, 2))
    outside = 0
    for i in range(n2):
        k = klR[i]
        vx = float(_f32(k["endPointX"] - k["startPointX"])) * iw
        vy = float(_f32(k["endPointY"] - k["startPointY"])) * ih
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.float64(math.sqrt(fma(vx, vx, vy * vy)))
            dirs[i] = (np.float64(vx) / m, np.float64(vy) / m)
        for (x, y) in line_iterator(float(k["startPointX"]) * iw, float(k["startPointY"]) * ih,
                                    float(k["endPointX"]) * iw, float(k["endPointY"]) * ih):
            if 0 <= x < 64 and 0 <= y < 48:
                grid[x][y].append(i)
            else:
                outside += 1
    _, m12 = oracle_lib.match_grid(lines1, dL, grid, dR, dirs, range_hint=range_hint)
    disp = np.full((n1, 2), -1, np.float32)
    dep = np.full((n1, 2), -1, np.float32)
    codes = np.full(n1, SL_UNMATCHED, np.int32)
    arms = np.full(n1, OV_NONE, np.int32)
    quirk = np.zeros(n1, bool)
    raw = np.full((n1, 2), np.nan)
    th = float(_f32(0.1))
    for i1 in range(n1):
        i2 = m12[i1]
        if i2 < 0:
            continue
        spl0, spl1, epl0, epl1 = sx[i1], sy[i1], ex[i1], ey[i1]
        r = klR[i2]
        spr0, spr1 = float(r["startPointX"]), float(r["startPointY"])
        epr0, epr1 = float(r["endPointX"]), float(r["endPointY"])
        right_flat = not abs(spr1 - epr1) > th
        ov, arms[i1] = py_overlap_traced(spl1, epl1, spr1, epr1)
        with np.errstate(divide="ignore", invalid="ignore"):
            plain = np.float64(fma(spr0, epl1 - epr1, epr0 * (spr1 - epl1))) / np.float64(spr1 - epr1)
            spr0 = float(np.float64(fma(spr0, spl1 - epr1, epr0 * (spr1 - spl1))) / np.float64(spr1 - epr1))
            spr1 = spl1
            epr0 = float(np.float64(fma(spr0, epl1 - epr1, epr0 * (spr1 - epl1))) / np.float64(spr1 - epr1))
            epr1 = epl1
            ds, de = spl0 - spr0, epl0 - epr0
            raw[i1] = (ds, de)
            de_plain = epl0 - float(plain)

            def filt(a, b):
                mn = b if b < a else a
                mx = b if a < b else a
                return (-1.0, -1.0) if np.float64(mn) / np.float64(mx) < float(_f32(0.7)) else (a, b)
            fs, fe = filt(ds, de)
            ps, pe = filt(ds, de_plain)
        geom = abs(spl1 - epl1) > th and abs(spr1 - epr1) > th and ov > float(_f32(0.75))
        ok = fs >= 1 and fe >= 1 and geom
        quirk[i1] = ok != (ps >= 1 and pe >= 1 and geom)
        if not abs(spl1 - epl1) > th:
            codes[i1] = SL_HORIZONTAL_LEFT
        elif right_flat:
            codes[i1] = SL_HORIZONTAL_RIGHT
        elif (fs, fe) != (ds, de) and not (np.isnan(ds) or np.isnan(de)):
            codes[i1] = SL_RATIO_REJECT
        elif not (fs >= 1 and fe >= 1):
            codes[i1] = SL_MIN_DISP_REJECT
        elif not ov > float(_f32(0.75)):
            codes[i1] = SL_OVERLAP_REJECT
        else:
            codes[i1] = SL_ACCEPTED
        if ok:
            disp[i1] = (fs, fe)
            dep[i1] = (_f32(mbf) / _f32(fs), _f32(mbf) / _f32(fe))
    le = np.zeros((n1, 3))
    if n2 > 0:
        un = klL if klUn is None else klUn
        for i in range(n1):
            a0, a1, b0, b1 = (float(un[f][i]) for f in ("startPointX", "startPointY", "endPointX", "endPointY"))
            l0, l1, l2 = a1 - b1, b0 - a0, fma(a0, b1, -(a1 * b0))  # Eigen cross + norm, fused in Frame.cc.o
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.float64(math.sqrt(fma(l0, l0, l1 * l1)))
                le[i] = (np.float64(l0) / s, np.float64(l1) / s, np.float64(l2) / s)
    info = {"arm": arms, "le": le, "grid_total": sum(len(c) for col in grid for c in col), "cells_outside": outside,
            "max_cell": max(len(c) for col in grid for c in col), "quirk": quirk, "disp": raw}
    return m12, disp, dep, codes, info


def py_stereo_lines(klL, dL, klR, dR, W, H, mbf):
    """(matches_12, mvDisparity_l, mvDepth_l) of py_stereo_lines_traced."""
    return py_stereo_lines_traced(klL, dL, klR, dR, W, H, mbf)[:3]


def flip_bits(desc, k, rng):
    """A copy of the 32-byte descriptor with exactly k of its 256 bits flipped."""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def stereo_lds_bytes(n_rows, cap_l, cap_r, nlevels, sf=1.2):
    """Dynamic LDS of stereo_orb_kernel (Stereo): row offsets and cursors, right u / octave, four
    per-left-keypoint tables and the row buckets of cap_r * (ceil(4 * scale_top) + 3) 16-bit entries."""
    top = orb_scale_factors(nlevels, sf)[nlevels - 1]
    row_cap = cap_r * (int(math.ceil(np.float32(2) * (np.float32(2.0) * top))) + 3)
    return (2 * n_rows + 1) * 4 + 8 * cap_r + 16 * cap_l + (2 * row_cap + 15) // 16 * 16


class StereoScene:
    """A hand-made rectified ORB pair for Frame::ComputeStereoMatches: per level a random left plane and a
    right plane holding the same content moved `shift` pixels to the left (right[y, x] = left[y, x + shift];
    an int, or one int per row of the level) plus uniform noise of amplitude `noise` (an int, or one per row);
    the planes are no resizes of each other, the matcher only reads them.  fold = P makes every row of both
    planes a triangle-wave fold of a random base (img[:, x] = base[:, |((x + P) mod 2P) - P|]), so that every
    column that is a multiple of P is a mirror axis.  Keypoints are placed by hand (add_*); a matching pair
    shares a random descriptor, unrelated ones sit near distance 128."""

    def __init__(self, seed, nlevels, w0=160, h0=96, shift=3, noise=3, sizes=None, fold=None):
        from oracle_lib import KEYPOINT_DTYPE
        self.dtype = KEYPOINT_DTYPE
        self.rng = rng = np.random.default_rng(seed)
        self.n = nlevels
        self.scale = orb_scale_factors(nlevels)
        self.inv = np.zeros(16, np.float32)
        self.inv[:nlevels] = [np.float32(1.0) / s for s in self.scale[:nlevels]]
        self.sizes = sizes or [(int(round(w0 / float(self.scale[lv]))), int(round(h0 / float(self.scale[lv]))))
                               for lv in range(nlevels)]
        self.pL, self.pR, self.shift = [], [], []
        for lv, (w, h) in enumerate(self.sizes):
            sh = shift[lv] if isinstance(shift, (list, tuple)) else shift
            sh = np.broadcast_to(np.asarray(sh, np.int64), (h,))
            nz = noise[lv] if isinstance(noise, (list, tuple)) else noise
            nz = np.broadcast_to(np.asarray(nz, np.int64), (h,))
            self.shift.append(sh)
            if fold:
                base = rng.integers(0, 256, (h, fold + 1), dtype=np.uint8)
                tri = np.abs((np.arange(w) + fold) % (2 * fold) - fold)
                nb = np.clip(base.astype(np.int64) + (rng.integers(-1, 2, base.shape) * nz[:, None]), 0, 255)
                self.pL.append(np.ascontiguousarray(base[:, tri]))
                self.pR.append(np.ascontiguousarray(nb.astype(np.uint8)[:, tri]))
                continue
            left = rng.integers(0, 256, (h, w), dtype=np.uint8)
            right = rng.integers(0, 256, (h, w), dtype=np.uint8)
            xs = np.arange(w)[None, :] + sh[:, None]
            ok = (xs >= 0) & (xs < w)
            moved = np.take_along_axis(left, np.clip(xs, 0, w - 1), 1)
            right = np.where(ok, moved, right).astype(np.int64)
            right = right + (rng.integers(-1, 2, (h, w)) * nz[:, None])
            self.pL.append(left)
            self.pR.append(np.clip(right, 0, 255).astype(np.uint8))
        self.kl, self.dl, self.kr, self.dr = [], [], [], []

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def add_left(self, x, y, octave, desc):
        self.kl.append((np.float32(x), np.float32(y), octave))
        self.dl.append(np.asarray(desc, np.uint8))
        return len(self.kl) - 1

    def add_right(self, x, y, octave, desc):
        self.kr.append((np.float32(x), np.float32(y), octave))
        self.dr.append(np.asarray(desc, np.uint8))
        return len(self.kr) - 1

    def level_xy(self, xl, yl, octave):
        """Image coordinates of the level pixel (xl, yl): round(x * mvInvScaleFactors) gives it back."""
        s = self.scale[octave]
        x, y = np.float32(np.float32(xl) * s), np.float32(np.float32(yl) * s)
        back = (round(float(np.float32(x * self.inv[octave]))), round(float(np.float32(y * self.inv[octave]))))
        assert back == (xl, yl)
        return x, y

    def add_pair(self, xl, yl, octave, e=0, flips=0):
        """A left keypoint on level pixel (xl, yl) and its right keypoint listed e level pixels to the right
        of where the content is (the SAD minimum then lies at incR = -e); the right descriptor differs in
        `flips` bits."""
        x, y = self.level_xy(xl, yl, octave)
        xr, _ = self.level_xy(xl - int(self.shift[octave][yl]) + e, yl, octave)
        d = self.desc()
        return self.add_left(x, y, octave, d), self.add_right(xr, y, octave, flip_bits(d, flips, self.rng))

    def tables(self):
        def tab(k):
            t = np.zeros(len(k), self.dtype)
            for i, (x, y, o) in enumerate(k):
                t["x"][i], t["y"][i], t["octave"][i] = x, y, o
            t["size"], t["class_id"] = 31, -1
            return t
        return (tab(self.kl), np.array(self.dl, np.uint8).reshape(-1, 32), tab(self.kr),
                np.array(self.dr, np.uint8).reshape(-1, 32), self.pL, self.pR, self.scale, self.inv)


class StereoLineSet:
    """Hand-built keylines for Frame::ComputeStereoMatches_Lines: only the end points and the LBD descriptors
    are read.  A pair shares a random descriptor (distance 0, every other line near 128), so matchGrid pairs
    them whenever the right line crosses the grid window of a left end point."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.L, self.R, self.dl, self.dr, self.un = [], [], [], [], []

    def left(self, line, desc=None, un=None):
        self.L.append(line)
        self.un.append(un if un is not None else (line[0] + 0.25, line[1], line[2], line[3]))
        self.dl.append(self.rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc)
        return len(self.L) - 1

    def right(self, line, desc=None):
        self.R.append(line)
        self.dr.append(self.rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc)
        return len(self.R) - 1

    def pair(self, left, right, un=None):
        d = self.rng.integers(0, 256, 32, dtype=np.uint8)
        return self.left(left, d, un), self.right(right, d.copy())

    def tables(self):
        from oracle_lib import KEYLINE_DTYPE

        def tab(lines):
            t = np.zeros(len(lines), KEYLINE_DTYPE)
            for i, ln in enumerate(lines):
                (t["startPointX"][i], t["startPointY"][i], t["endPointX"][i], t["endPointY"][i]) = ln
            return t
        return (tab(self.L), np.array(self.dl, np.uint8).reshape(-1, 32), tab(self.R),
                np.array(self.dr, np.uint8).reshape(-1, 32), tab(self.un))


# ------------------------------------------------- the tracking projection matchers (csrc/proj.hip), traced
# Pure-Python restatements of the five guided searches of tracking, written from the reference lines, each
# sequential like the reference:
#   py_proj_traced   SearchByProjection(CurrentFrame, LastFrame, th, bMono)   ORBmatcher.cc:1962-2178, one camera
#                    (Nleft == -1) and two cameras (:1985-2153)
#   py_local_traced  SearchByProjection(F, vpMapPoints, th, ...)               ORBmatcher.cc:44-143 and :44-214
#   py_reloc_traced  SearchByProjection(CurrentFrame, pKF, sAlreadyFound, ...) ORBmatcher.cc:2180-2300
# over one GetFeaturesInArea walker (Frame.cc:1006-1075, pj_in_area) and ComputeThreeMaxima (ORBmatcher.cc:
# 2304-2345, py_three_maxima).  Every one returns (nmatches, [match table per image], trace): per image and
# point a set of PJ_* outcome codes, the scan against the flags on entry ("p1": what phase 1 of the kernels
# computes) and against the flags at the point's turn ("fin"), the rotation histogram and the kept bins.
# `mut` switches one deliberate mistake on (PJ_MUTANTS); tests/test_proj_branches.py uses it to prove that
# the crafted inputs tell that mistake from the reference behaviour.
PJ_NAMES = ("NOT_SEARCHED", "BAD_LEVEL", "BEHIND", "OUT_OF_BOUNDS", "DEPTH_RANGE", "WINDOW_RIGHT", "WINDOW_LEFT",
            "WINDOW_BELOW", "WINDOW_ABOVE", "EMPTY_WINDOW", "ALL_BLOCKED", "OVER_THRESHOLD", "RATIO_REJECTED",
            "ACCEPTED", "ACCEPTED_BY_LEVEL", "ACCEPTED_AFTER_RESCAN", "LOST_AFTER_RESCAN", "OVERWROTE", "MIRRORED",
            "UNBLOCKED_PARTNER", "ROT_DROPPED", "SIDE_SKIPPED")
(PJ_NOT_SEARCHED, PJ_BAD_LEVEL, PJ_BEHIND, PJ_OUT_OF_BOUNDS, PJ_DEPTH_RANGE, PJ_WINDOW_RIGHT, PJ_WINDOW_LEFT,
 PJ_WINDOW_BELOW, PJ_WINDOW_ABOVE, PJ_EMPTY_WINDOW, PJ_ALL_BLOCKED, PJ_OVER_THRESHOLD, PJ_RATIO_REJECTED,
 PJ_ACCEPTED, PJ_ACCEPTED_BY_LEVEL, PJ_ACCEPTED_AFTER_RESCAN, PJ_LOST_AFTER_RESCAN, PJ_OVERWROTE, PJ_MIRRORED,
 PJ_UNBLOCKED_PARTNER, PJ_ROT_DROPPED, PJ_SIDE_SKIPPED) = range(len(PJ_NAMES))
PJ_WINDOW_RETURNS = (PJ_WINDOW_RIGHT, PJ_WINDOW_LEFT, PJ_WINDOW_BELOW, PJ_WINDOW_ABOVE)  # in the reference's order
PJ_TAKEN = (PJ_ACCEPTED, PJ_ACCEPTED_BY_LEVEL)
# no phase-2 re-scan / re-scan when the best was taken only / no `unblocked` handling / ties to the lowest index /
# |dx| <= radius / er >= radius / ratio product in double / rint bin / >= in ComputeThreeMaxima / <= in its 10 %
# cut / one decrement per nulled keypoint / bestDist < TH_HIGH
PJ_MUTANTS = ("no_rescan", "rescan_best_only", "no_unblocked", "low_index_tie", "le_radius", "ge_uright",
              "ratio_double", "rint_bin", "ge_three_maxima", "le_ten_percent", "dec_per_keypoint", "lt_th_high")
TM_BRANCHES = ("first", "second", "third", "cut_two", "cut_third", "keep_three")
PJ_TH_HIGH, PJ_HISTO = 100, 30


def _libm_f32(name, nargs):
    import ctypes
    import ctypes.util
    fn = getattr(ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6"), name)
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float] * nargs
    return lambda *a: np.float32(fn(*(float(t) for t in a)))


def pj_project(camera, kb8, x, y, z):
    """Pinhole::project (Pinhole.cpp:30-33) or KannalaBrandt8::project (KannalaBrandt8.cpp:33-48, the host
    libm and the fused sites of oracle/proj_oracle.cpp) on float32."""
    f = np.float32
    fx, fy, cx, cy = (f(t) for t in camera[:4])
    x, y, z = f(x), f(y), f(z)
    if kb8 is None:
        return f(f(f(fx * x) / z) + cx), f(f(f(fy * y) / z) + cy)
    atan2f, cosf, sinf = _libm_f32("atan2f", 2), _libm_f32("cosf", 1), _libm_f32("sinf", 1)
    k = [f(t) for t in kb8]
    theta = atan2f(np.sqrt(fmaf(x, x, f(y * y))), z)
    psi = atan2f(y, x)
    t2 = f(theta * theta)
    t3 = f(theta * t2)
    t5 = f(t3 * t2)
    t7 = f(t5 * t2)
    t9 = f(t7 * t2)
    r = fmaf(k[3], t9, fmaf(k[2], t7, fmaf(k[1], t5, fmaf(k[0], t3, theta))))
    return fmaf(f(fx * r), cosf(psi), cx), fmaf(f(fy * r), sinf(psi), cy)


def pj_window(grid, x, y, r):
    """The cell range of GetFeaturesInArea (Frame.cc:1013-1037): ((x0, x1, y0, y1), 0), or (None, k) where the
    reference returns early at its k-th test (1..4)."""
    f = np.float32
    min_x, _, min_y, _, inv_w, inv_h = (f(t) for t in grid)
    x, y, r = f(x), f(y), f(r)
    x0 = max(0, math.floor(f(f(f(x - min_x) - r) * inv_w)))
    if x0 >= 64:
        return None, 1
    x1 = min(63, math.ceil(f(f(f(x - min_x) + r) * inv_w)))
    if x1 < 0:
        return None, 2
    y0 = max(0, math.floor(f(f(f(y - min_y) - r) * inv_h)))
    if y0 >= 48:
        return None, 3
    y1 = min(47, math.ceil(f(f(f(y - min_y) + r) * inv_h)))
    if y1 < 0:
        return None, 4
    return (x0, x1, y0, y1), 0


def pj_in_area(cells, k, grid, x, y, r, lo, hi, mut=()):
    """GetFeaturesInArea(x, y, r, lo, hi) -> (vIndices in the reference's order, early-return number)."""
    f = np.float32
    win, ret = pj_window(grid, x, y, r)
    if win is None:
        return [], ret
    x, y, r = f(x), f(y), f(r)
    check = lo > 0 or hi >= 0
    le = "le_radius" in mut
    out = []
    for ix in range(win[0], win[1] + 1):
        for iy in range(win[2], win[3] + 1):
            for i in cells[ix][iy]:
                o = int(k["octave"][i])
                if check and (o < lo or (hi >= 0 and o > hi)):
                    continue
                dx, dy = abs(f(k["x"][i] - x)), abs(f(k["y"][i] - y))
                if (dx <= r and dy <= r) if le else (dx < r and dy < r):
                    out.append(i)
    return out, 0


def py_rot_bin(a, b, mut=()):
    """The rotation-histogram bin of a - b (ORBmatcher.cc:2071-2077): float factor 1.0f / HISTO_LENGTH, round()."""
    f = np.float32
    rot = f(f(a) - f(b))
    if rot < 0:
        rot = f(rot + f(360.0))
    v = f(rot * f(f(1.0) / f(PJ_HISTO)))
    b_ = int(np.rint(v)) if "rint_bin" in mut else int(math.floor(float(v) + 0.5))  # v >= 0: half away from zero
    return 0 if b_ == PJ_HISTO else b_


def py_three_maxima(hist, mut=()):
    """ComputeThreeMaxima (ORBmatcher.cc:2304-2345) on the bin counts -> ((ind1, ind2, ind3), branches taken)."""
    f = np.float32
    ge, le = "ge_three_maxima" in mut, "le_ten_percent" in mut
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    taken = set()
    for i, s in enumerate(hist):
        if (s >= max1) if ge else (s > max1):
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
            taken.add("first")
        elif (s >= max2) if ge else (s > max2):
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
            taken.add("second")
        elif (s >= max3) if ge else (s > max3):
            max3, ind3 = s, i
            taken.add("third")
    lim = f(f(0.1) * f(max1))

    def cut(m):
        return f(m) <= lim if le else f(m) < lim
    if cut(max2):
        ind2 = ind3 = -1
        taken.add("cut_two")
    elif cut(max3):
        ind3 = -1
        taken.add("cut_third")
    else:
        taken.add("keep_three")
    return (ind1, ind2, ind3), taken


class _PjSide:
    """One image of the frame: mvKeys(Un), the grid, mvpMapPoints as (match, blocked)."""

    def __init__(self, kps, desc, blocked, grid, mp_desc):
        from batch_pack import hamming
        from test_projection import _py_grid
        self.k, self.n = kps, len(kps)
        self.cells = _py_grid(kps["x"], kps["y"], grid)
        self.pre = np.zeros(self.n, bool) if blocked is None else np.asarray(blocked).astype(bool)
        self.blk = self.pre.copy()
        self.match = np.full(self.n, -1, np.int32)
        self.nulled = np.zeros(self.n, bool)
        self.oct = kps["octave"]
        self.dist = hamming(mp_desc, desc) if self.n and len(mp_desc) else np.zeros((len(mp_desc), self.n), np.int32)

    def table(self):
        return np.where(self.nulled, -2, self.match).astype(np.int32)


def _pj_scan(idxs, blk, drow, reject, mut):
    """The candidate loop: first argmin and first argmin of the rest, in vIndices order."""
    bd, bi, bd2, bi2 = 256, -1, 256, -1
    for i in (sorted(idxs) if "low_index_tie" in mut else idxs):
        if blk[i] or (reject is not None and reject(i)):
            continue
        d = int(drow[i])
        if d < bd:
            bd2, bi2, bd, bi = bd, bi, d, i
        elif d < bd2:
            bd2, bi2 = d, i
    return bd, bi, bd2, bi2


def _pj_pick(side, idxs, drow, reject, two, mut):
    """(p1, fin): the scan against the flags on entry and the one the point's turn gets.  The reference is
    sequential, so fin is the scan against the current flags; the schedule mutants keep p1 where a kernel with
    that mistake would."""
    p1 = _pj_scan(idxs, side.pre, drow, reject, mut)
    seq = _pj_scan(idxs, side.blk, drow, reject, mut)

    def moved(i):
        return i >= 0 and side.blk[i] != side.pre[i]
    if "no_rescan" in mut:
        fin = p1
    elif "rescan_best_only" in mut:
        fin = seq if moved(p1[1]) else p1
    elif "no_unblocked" in mut:
        fin = seq if moved(p1[1]) or (two and moved(p1[3])) else p1
    else:
        fin = seq
    if not two:
        p1, fin = p1[:2] + (256, -1), fin[:2] + (256, -1)
    return p1, fin


def _pj_trace(sides, n):
    return {"codes": [[set() for _ in range(n)] for _ in sides], "p1": [[None] * n for _ in sides],
            "fin": [[None] * n for _ in sides], "rescans": [], "verdicts": set(), "window_returns": set(),
            "hist": [0] * PJ_HISTO, "keep": None, "three_maxima": set(), "entries": []}


def _pj_record(tr, s, i, p1, fin, v1, vf):
    tr["p1"][s][i], tr["fin"][s][i] = p1, fin
    tr["codes"][s][i].add(vf)
    if p1 != fin:
        tr["rescans"].append((s, i))
        tr["verdicts"].add((v1, vf))
        if vf in PJ_TAKEN:
            tr["codes"][s][i].add(PJ_ACCEPTED_AFTER_RESCAN)
        elif v1 in PJ_TAKEN:
            tr["codes"][s][i].add(PJ_LOST_AFTER_RESCAN)


def _pj_empty(tr, s, i, ret):
    tr["codes"][s][i].add(PJ_WINDOW_RETURNS[ret - 1] if ret else PJ_EMPTY_WINDOW)
    if ret:
        tr["window_returns"].add(ret)


def _pj_verdict_one(t, thr, mut):
    if t[1] < 0:
        return PJ_ALL_BLOCKED
    return PJ_ACCEPTED if (t[0] < thr if "lt_th_high" in mut else t[0] <= thr) else PJ_OVER_THRESHOLD


def _pj_verdict_two(t, side, nnratio, mut):
    """The level-aware ratio test of the local search (ORBmatcher.cc:124-129): a float product."""
    bd, bi, bd2, bi2 = t
    if bi < 0:
        return PJ_ALL_BLOCKED
    if not (bd < PJ_TH_HIGH if "lt_th_high" in mut else bd <= PJ_TH_HIGH):
        return PJ_OVER_THRESHOLD
    lvl, lvl2 = int(side.oct[bi]), (int(side.oct[bi2]) if bi2 >= 0 else -1)
    if "ratio_double" in mut:
        fails = bd > float(np.float32(nnratio)) * bd2
    else:
        fails = np.float32(bd) > np.float32(np.float32(nnratio) * np.float32(bd2))
    if lvl == lvl2 and fails:
        return PJ_RATIO_REJECTED
    return PJ_ACCEPTED_BY_LEVEL if bi2 >= 0 and fails else PJ_ACCEPTED


def _pj_store(tr, sides, s, i, bi, obs):
    side = sides[s]
    if side.match[bi] >= 0:
        tr["codes"][s][i].add(PJ_OVERWROTE)
    side.match[bi] = i
    side.blk[bi] = bool(obs)


def _pj_rotation(tr, sides, nm, check_ori, mut):
    """The rotation filter (ORBmatcher.cc:2155-2175 / :2284-2296): every entry of a dropped bin NULLs its keypoint
    and decrements nmatches."""
    if not check_ori:
        return nm
    for s, bi, b, i in tr["entries"]:
        tr["hist"][b] += 1
    keep, taken = py_three_maxima(tr["hist"], mut)
    tr["keep"], tr["three_maxima"] = keep, taken
    dropped = [(s, bi, i) for s, bi, b, i in tr["entries"] if b not in keep]
    for s, bi, i in dropped:
        sides[s].nulled[bi] = True
        tr["codes"][s][i].add(PJ_ROT_DROPPED)
    return nm - (len({(s, bi) for s, bi, _ in dropped}) if "dec_per_keypoint" in mut else len(dropped))


def _pj_levels(forward, backward, L):
    if forward:
        return L, -1
    if backward:
        return 0, L
    return L - 1, L + 1


def py_proj_traced(case, th, forward=0, backward=0, check_ori=1, mut=(), nlevels=8):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono): one camera (case keys of util.projection_case) or
    two (util.projection_stereo_case)."""
    f = np.float32
    c = case
    two = "kps_r" in c
    grid, sf, md = c["grid"], c["scale_factors"], c["mp_desc"]
    if two:
        sides = [_PjSide(c["kps"], c["desc"], c["blocked"], grid, md),
                 _PjSide(c["kps_r"], c["desc_r"], c["blocked_r"], grid, md)]
        uright = None
    else:
        sides = [_PjSide(c["cur_kps"], c["cur_desc"], c["cur_blocked"], grid, md)]
        uright = c.get("cur_uright")
    min_x, max_x, min_y, max_y = (f(t) for t in grid[:4])
    n = len(c["flags"])
    tr = _pj_trace(sides, n)
    nm = 0
    for i in range(n):
        cs = [tr["codes"][s][i] for s in range(len(sides))]
        if not c["flags"][i] & 1:
            for s_ in cs:
                s_.add(PJ_NOT_SEARCHED)
            continue
        obs = bool(c["flags"][i] & 2)
        xc, yc, zc = (f(t) for t in c["x3dc"][i])
        invzc = f(1.0 / float(zc))
        if invzc < 0:
            cs[0].add(PJ_BEHIND)
            continue
        u, v = pj_project(c["camera"], c.get("kb8") if two else None, xc, yc, zc)
        if u < min_x or u > max_x or v < min_y or v > max_y:
            cs[0].add(PJ_OUT_OF_BOUNDS)
            continue
        L = int(c["last_octave"][i])
        if L < 0 or L >= nlevels:
            cs[0].add(PJ_BAD_LEVEL)
            continue
        radius = f(f(th) * f(sf[L]))
        lo, hi = _pj_levels(forward, backward, L)
        for s, side in enumerate(sides):
            if s == 1:
                u, v = pj_project(c["camera"], c.get("kb8"), *c["x3dr"][i])
            idxs, ret = pj_in_area(side.cells, side.k, grid, u, v, radius, lo, hi, mut)
            if not idxs:
                _pj_empty(tr, s, i, ret)
                if s == 0:  # `continue` at :2035: the right image is not searched either
                    if two:
                        cs[1].add(PJ_SIDE_SKIPPED)
                    break
                continue
            reject = None
            if uright is not None:
                ur = fmaf(-f(c["camera"][4]), invzc, u)  # fused in the reference object, as the oracle has it

                def reject(i2, ur=ur):
                    if not uright[i2] > 0:
                        return False
                    er = abs(f(ur - f(uright[i2])))
                    return er >= radius if "ge_uright" in mut else er > radius
            p1, fin = _pj_pick(side, idxs, side.dist[i], reject, False, mut)
            v1, vf = _pj_verdict_one(p1, PJ_TH_HIGH, mut), _pj_verdict_one(fin, PJ_TH_HIGH, mut)
            _pj_record(tr, s, i, p1, fin, v1, vf)
            if vf == PJ_ACCEPTED:
                _pj_store(tr, sides, s, i, fin[1], obs)
                nm += 1
                if check_ori:
                    tr["entries"].append((s, fin[1], py_rot_bin(c["last_angle"][i], side.k["angle"][fin[1]], mut), i))
    nm = _pj_rotation(tr, sides, nm, check_ori, mut)
    return nm, [s.table() for s in sides], tr


def py_reloc_traced(case, th, orb_dist, check_ori=1, mut=(), nlevels=8):
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (case keys of util.reloc_case)."""
    f = np.float32
    c = case
    grid, sf = c["grid"], c["scale_factors"]
    sides = [_PjSide(c["cur_kps"], c["cur_desc"], c["cur_blocked"], grid, c["mp_desc"])]
    side = sides[0]
    min_x, max_x, min_y, max_y = (f(t) for t in grid[:4])
    n = len(c["kf_flags"])
    tr = _pj_trace(sides, n)
    nm = 0
    for i in range(n):
        cs = tr["codes"][0][i]
        if not c["kf_flags"][i] & 1:
            cs.add(PJ_NOT_SEARCHED)
            continue
        u, v = pj_project(c["camera"], None, *c["x3dc"][i])  # no depth test (:2205-2212)
        if u < min_x or u > max_x or v < min_y or v > max_y:
            cs.add(PJ_OUT_OF_BOUNDS)
            continue
        d3, dmin, dmax = (f(t) for t in c["dist"][i])
        if d3 < dmin or d3 > dmax:
            cs.add(PJ_DEPTH_RANGE)
            continue
        L = int(c["level"][i])
        if L < 0 or L >= nlevels:
            cs.add(PJ_BAD_LEVEL)
            continue
        radius = f(f(th) * f(sf[L]))
        idxs, ret = pj_in_area(side.cells, side.k, grid, u, v, radius, L - 1, L + 1, mut)
        if not idxs:
            _pj_empty(tr, 0, i, ret)
            continue
        p1, fin = _pj_pick(side, idxs, side.dist[i], None, False, mut)
        v1, vf = _pj_verdict_one(p1, orb_dist, mut), _pj_verdict_one(fin, orb_dist, mut)
        _pj_record(tr, 0, i, p1, fin, v1, vf)
        if vf == PJ_ACCEPTED:
            _pj_store(tr, sides, 0, i, fin[1], True)
            nm += 1
            if check_ori:
                tr["entries"].append((0, fin[1], py_rot_bin(c["kf_angle"][i], side.k["angle"][fin[1]], mut), i))
    nm = _pj_rotation(tr, sides, nm, check_ori, mut)
    return nm, [side.table()], tr


def py_local_traced(case, th, nnratio=0.8, mut=(), nlevels=8):
    """SearchByProjection(F, vpMapPoints, th, ...): one camera (case keys of util.local_case) or two
    (util.local_stereo_case)."""
    f = np.float32
    c = case
    two = "kps_r" in c
    grid, sf, md = c["grid"], c["scale_factors"], c["mp_desc"]
    if two:
        sides = [_PjSide(c["kps"], c["desc"], c["blocked"], grid, md),
                 _PjSide(c["kps_r"], c["desc_r"], c["blocked_r"], grid, md)]
        proj, lvl, pair, uright = (c["mp_proj"], c["mp_proj_r"]), (c["mp_level"], c["mp_level_r"]), \
            (c["l2r"], c["r2l"]), None
    else:
        sides = [_PjSide(c["cur_kps"], c["cur_desc"], c["cur_blocked"], grid, md)]
        proj, lvl, pair, uright = (c["mp_proj"],), (c["mp_level"],), (None,), c.get("cur_uright")
    n = len(c["mp_flags"])
    tr = _pj_trace(sides, n)
    nm = 0
    for m in range(n):
        fl = int(c["mp_flags"][m])
        obs = bool(fl & 2)
        for s, side in enumerate(sides):
            cs = tr["codes"][s][m]
            if not fl & (1, 4)[s]:
                cs.add(PJ_NOT_SEARCHED)
                continue
            L = int(lvl[s][m])
            if L < 0 or L >= nlevels:
                cs.add(PJ_BAD_LEVEL)
                continue
            x, y, xr, vcos = (f(t) for t in proj[s][m])
            r = f(2.5) if float(vcos) > 0.998 else f(4.0)  # RadiusByViewingCos (:216-222)
            if s == 0 and float(f(th)) != 1.0:
                r = f(r * f(th))
            radius = f(r * f(sf[L]))
            idxs, ret = pj_in_area(side.cells, side.k, grid, x, y, radius, L - 1, L, mut)
            if not idxs:
                _pj_empty(tr, s, m, ret)
                continue
            reject = None
            if uright is not None:
                def reject(i2, xr=xr, radius=radius):
                    if not uright[i2] > 0:
                        return False
                    er = abs(f(xr - f(uright[i2])))
                    return er >= radius if "ge_uright" in mut else er > radius
            p1, fin = _pj_pick(side, idxs, side.dist[m], reject, True, mut)
            v1, vf = _pj_verdict_two(p1, side, nnratio, mut), _pj_verdict_two(fin, side, nnratio, mut)
            _pj_record(tr, s, m, p1, fin, v1, vf)
            if vf == PJ_RATIO_REJECTED:
                if two and s == 0 and fl & 4:
                    tr["codes"][1][m].add(PJ_SIDE_SKIPPED)
                break  # the `continue` at :127 / :197: the next MapPoint
            if vf in PJ_TAKEN:
                _pj_store(tr, sides, s, m, fin[1], obs)
                nm += 1
                o = int(pair[s][fin[1]]) if pair[s] is not None else -1
                if o != -1:  # the stereo observation in the other image (:132-136 / :199-203), unchecked
                    other = sides[1 - s]
                    cs.add(PJ_MIRRORED)
                    if other.blk[o] and not obs:
                        cs.add(PJ_UNBLOCKED_PARTNER)
                    other.match[o] = m
                    other.blk[o] = obs
                    nm += 1
    return nm, [s.table() for s in sides], tr


class ProjScene:
    """Hand-placed inputs of one of the five searches (kind: "proj", "proj2", "local", "local2", "reloc"), in the
    dict layout of the util.*_case generators.  Keypoints go where the builder puts them, descriptors are a
    random base with chosen bits flipped (flip / flip_at), so every Hamming distance is known.  The camera is
    fx = fy = 1, cx = cy = 0 unless given, and a point at depth z (a power of two) is x3Dc = (u z, v z, z): its
    projection is (u, v) exactly; mbf = 8, so ur = u - 8 / z."""
    KINDS = ("proj", "proj2", "local", "local2", "reloc")

    def __init__(self, kind, seed, W=752, H=480, uright=False, kb8=None, camera=None):
        from oracle_lib import KEYPOINT_DTYPE
        f = np.float32
        assert kind in self.KINDS
        self.kind, self.rng, self.dtype = kind, np.random.default_rng(seed), KEYPOINT_DTYPE
        self.two = kind in ("proj2", "local2")
        self.grid = (f(0), f(W), f(0), f(H), f(64) / f(W), f(48) / f(H))
        self.camera = camera or (f(1), f(1), f(0), f(0), f(8))
        self.kb8, self.uright = kb8, uright
        self.sf = orb_scale_factors()
        self.K, self.D, self.B, self.U, self.pairs = ([], []), ([], []), ([], []), [], []
        self.P = []
        self._opener = None

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flip(self, d, k):
        return flip_bits(d, k, self.rng)

    @staticmethod
    def flip_at(d, positions):
        bits = np.unpackbits(np.asarray(d, np.uint8))
        bits[list(positions)] ^= 1
        return np.packbits(bits)

    def kp(self, x, y, o=0, d=None, angle=0.0, blocked=0, ur=-1.0, side=0):
        self.K[side].append((np.float32(x), np.float32(y), int(o), np.float32(angle)))
        self.D[side].append(self.desc() if d is None else np.asarray(d, np.uint8))
        self.B[side].append(int(blocked))
        if side == 0:
            self.U.append(np.float32(ur))
        return len(self.K[side]) - 1

    def link(self, il, ir):
        """mvLeftToRightMatch[il] = ir and mvRightToLeftMatch[ir] = il."""
        self.pairs.append((il, ir))

    def opener(self):
        """A spot of the left image with one far-off keypoint per octave: a two-camera frame-to-frame point
        projected there has a non-empty left window (and no left match), so its right image is searched."""
        if self._opener is None:
            self._opener = (np.float32(700.0), np.float32(24.0))
            for o in range(8):
                self.kp(*self._opener, o=o)
        return self._opener

    def pt(self, u, v, L=0, d=None, angle=0.0, on=1, obs=1, z=1.0, right=None, xr=0.0, vcos=1.0,
           dist=(5.0, 2.5, 10.0), x3=None, x3r=None):
        """A LastFrame point / MapPoint / KF MapPoint projected at (u, v) (level L) and, in a two-camera kind, at
        right = (ur, vr[, Lr]) of the right image (local2: None = not in view there; proj2: None = (u, v))."""
        f = np.float32
        self.P.append({"u": f(u), "v": f(v), "L": int(L), "d": self.desc() if d is None else np.asarray(d, np.uint8),
                       "angle": f(angle), "on": int(on), "obs": int(obs), "z": f(z), "right": right, "xr": f(xr),
                       "vcos": f(vcos), "dist": dist, "x3": x3, "x3r": x3r})
        return len(self.P) - 1

    def _kps(self, side):
        k = np.zeros(len(self.K[side]), self.dtype)
        for i, (x, y, o, a) in enumerate(self.K[side]):
            k["x"][i], k["y"][i], k["octave"][i], k["angle"][i] = x, y, o, a
        k["size"], k["class_id"] = 31, -1
        return k

    def case(self):
        f = np.float32
        P, n = self.P, len(self.P)

        def col(key, dtype, tail=()):
            return np.array([p[key] for p in P], dtype).reshape((n,) + tail)

        def x3(p, uv):
            return (f(uv[0] * p["z"]), f(uv[1] * p["z"]), p["z"])
        desc = [np.array(d, np.uint8).reshape(-1, 32) for d in self.D]
        blk = [np.array(b, np.uint8) for b in self.B]
        c = {"kind": self.kind, "grid": self.grid, "scale_factors": self.sf, "mp_desc": col("d", np.uint8, (32,))}
        if self.two:
            c.update(kps=self._kps(0), desc=desc[0], blocked=blk[0], kps_r=self._kps(1), desc_r=desc[1],
                     blocked_r=blk[1])
        else:
            c.update(cur_kps=self._kps(0), cur_desc=desc[0], cur_blocked=blk[0])
            if self.kind != "reloc":
                c["cur_uright"] = np.array(self.U, np.float32) if self.uright else None
        flags = np.array([p["on"] | p["obs"] << 1 for p in P], np.uint8)
        if self.kind in ("proj", "proj2", "reloc"):
            c["camera"] = self.camera
            c["x3dc"] = np.array([p["x3"] if p["x3"] is not None else x3(p, (p["u"], p["v"])) for p in P],
                                 np.float32).reshape(n, 3)
        if self.kind in ("proj", "proj2"):
            c.update(flags=flags, last_octave=col("L", np.int32), last_angle=col("angle", np.float32))
        if self.kind == "proj2":
            c["x3dr"] = np.array([p["x3r"] if p["x3r"] is not None else
                                  x3(p, p["right"][:2] if p["right"] is not None else (p["u"], p["v"])) for p in P],
                                 np.float32).reshape(n, 3)
            c["kb8"] = None if self.kb8 is None else np.array(self.kb8, np.float32)
        if self.kind == "reloc":
            c.update(kf_flags=(flags & 1), level=col("L", np.int32), kf_angle=col("angle", np.float32),
                     dist=np.array([p["dist"] for p in P], np.float32).reshape(n, 3))
        if self.kind in ("local", "local2"):
            c.update(mp_flags=flags, mp_level=col("L", np.int32),
                     mp_proj=np.array([(p["u"], p["v"], p["xr"], p["vcos"]) for p in P], np.float32).reshape(n, 4))
        if self.kind == "local2":
            r = [p["right"] for p in P]
            c["mp_flags"] = flags | np.array([4 if t is not None else 0 for t in r], np.uint8)
            c["mp_proj_r"] = np.array([(t[0], t[1], 0.0, p["vcos"]) if t is not None else (0.0, 0.0, 0.0, 1.0)
                                       for t, p in zip(r, P)], np.float32).reshape(n, 4)
            c["mp_level_r"] = np.array([(t[2] if len(t) > 2 else p["L"]) if t is not None else -1
                                        for t, p in zip(r, P)], np.int32)
            c["l2r"] = np.full(len(self.K[0]), -1, np.int32)
            c["r2l"] = np.full(len(self.K[1]), -1, np.int32)
            for il, ir in self.pairs:
                c["l2r"][il], c["r2l"][ir] = ir, il
        return c


def pj_restate(case, call, mut=()):
    """The traced restatement of the case's kind; call = {th, forward, backward, ori, nnratio, orb_dist}."""
    if case["kind"] in ("proj", "proj2"):
        return py_proj_traced(case, call["th"], call["forward"], call["backward"], call["ori"], mut)
    if case["kind"] == "reloc":
        return py_reloc_traced(case, call["th"], call["orb_dist"], call["ori"], mut)
    return py_local_traced(case, call["th"], call["nnratio"], mut)


def pj_oracle(case, call):
    """The C++ oracle's answer in the same form: (nmatches, [tables])."""
    import oracle_lib
    kind = case["kind"]
    if kind == "proj":
        r = oracle_lib.search_by_projection(case, call["th"], call["forward"], call["backward"], call["ori"])
    elif kind == "proj2":
        r = oracle_lib.search_by_projection_stereo(case, call["th"], call["forward"], call["backward"], call["ori"])
    elif kind == "reloc":
        r = oracle_lib.search_reloc(case, call["th"], call["orb_dist"], call["ori"])
    elif kind == "local":
        r = oracle_lib.search_local(case, call["th"], call["nnratio"])
    else:
        r = oracle_lib.search_local_stereo(case, call["th"], call["nnratio"])
    return r[0], list(r[1:])
